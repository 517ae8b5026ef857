"""Host side of the per-model physics kernels (csrc/avsim_phys_spec.hip), no GPU:

* csrc/avsim_phys_specs.h is what tools/gen_phys_specs.py writes today: the generator (PhysHost::build without a device, built with
  -fsanitize=address,undefined on the host side) is rebuilt in a temporary directory and its output compared with the committed header --
  a model or a table added to the image without regenerating the header fails here (on the device such a handle just takes the generic kernel);
* make_layout_of evaluated by the compiler (what a specialised kernel gets) equals make_layout_of at run time (what a handle gets), for
  the dims of every committed model, both capacity tiers and both sizes of real: a stand-alone program with static constexpr layouts,
  compiled with -fsanitize=address,undefined, compares them word by word against calls whose arguments the optimiser cannot see."""
import glob
import importlib.util
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "av_aloha_amd", "csrc")
CAP_EFC, CAP_CON = (176, 176, 336, 480, 176), (48, 48, 72, 96, 48)         # PhysHost::init's tables (avsim_phys_layout.h), checked below
CAP_EFC1, CAP_CON1 = (176, 176, 224, 288, 176), (48, 48, 56, 64, 48)


def _generator():
    spec = importlib.util.spec_from_file_location("gen_phys_specs", os.path.join(ROOT, "tools", "gen_phys_specs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_spec_header_is_what_the_generator_writes(tmp_path):
    gen = _generator()
    out = gen.generate(str(tmp_path / "avsim_phys_specs.h"), str(tmp_path), sanitize=True)
    with open(out) as f, open(gen.HEADER) as g:
        assert f.read() == g.read(), "csrc/avsim_phys_specs.h is stale: run python tools/gen_phys_specs.py"
    for _, model in gen.SPECS:
        assert os.path.exists(os.path.join(ROOT, "models", model + ".avm"))


PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "avsim_phys_layout.h"
using namespace avs;
struct Case { const char* name; int a[12]; };
template <int... A> struct CT { static constexpr Layout lay = make_layout_of(A...); };
static int bad = 0, seen = 0;
template <int... A> static void check(const char* name) {
    volatile int v[12] = {A...};      // run time: the optimiser cannot fold the call
    const Layout r = make_layout_of(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]);
    static constexpr Layout c = CT<A...>::lay;
    static_assert(c.nreal % 4 == 0 && c.nint % 4 == 0 && c.bytes_per_env % 16 == 0 && c.bytes_per_env >= c.nreal * 4 + c.nint * 4, "alignment");
    static_assert(c.qpos == 0 && c.U <= c.cdist && c.rowS == c.scr && c.rowS % 4 == 0 && c.Minv % 4 == 0, "record");
    seen++;
    if (std::memcmp(&r, &c, sizeof(Layout)) != 0) {
        bad++;
        const int *x = reinterpret_cast<const int*>(&r), *y = reinterpret_cast<const int*>(&c);
        for (int k = 0; k < LAYOUT_WORDS; k++) if (x[k] != y[k]) std::printf("%s: word %d run time %d, compile time %d\n", name, k, x[k], y[k]);
    }
}
int main() {
    static_assert(sizeof(Layout) == LAYOUT_WORDS * sizeof(int) && sizeof(MOff) == MOFF_WORDS * sizeof(int), "no padding");
    const int caps[4][5] = {@CAPS@};
    if (std::memcmp(caps[0], CAP_EFC, sizeof(CAP_EFC)) || std::memcmp(caps[1], CAP_CON, sizeof(CAP_CON)) || std::memcmp(caps[2], CAP_EFC1, sizeof(CAP_EFC1)) ||
        std::memcmp(caps[3], CAP_CON1, sizeof(CAP_CON1))) { std::printf("capacity tables differ from the test's\n"); return 1; }
@CHECKS@
    std::printf("layouts checked: %d, mismatches: %d\n", seen, bad);
    return bad ? 1 : 0;
}
"""


def _model_dims():
    from av_aloha_amd.compiler.compile import read_blob
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "models", "*.avm"))):
        md = read_blob(path)
        s = lambda k: int(np.asarray(md[k]).reshape(-1)[0])
        msize = int((np.asarray(md["tree_dofnum"]).astype(np.int64) ** 2).sum())
        out.append((os.path.basename(path)[:-4], s("task_id"), (s("nq"), s("nv"), s("nu"), s("nbody"), s("ngeom"), msize, s("ntree"))))
    return out


def test_constexpr_layout_equals_runtime_layout_for_every_model(tmp_path):
    models = _model_dims()
    assert len(models) >= 15 and any(m[0] == "slot_insertion_3arms" for m in models)
    checks = []
    for name, task, dims in models:
        for rb in (4, 8):
            # full tier (the second pass: its own capacities = the full ones) and first tier (smaller record, full strides)
            for con, efc in {(CAP_CON[task], CAP_EFC[task]), (CAP_CON1[task], CAP_EFC1[task])}:
                args = (con, efc, CAP_CON[task], CAP_EFC[task]) + dims + (rb,)
                checks.append('    check<%s>("%s");' % (", ".join(map(str, args)), name))
    caps = ", ".join("{" + ", ".join(map(str, c)) + "}" for c in (CAP_EFC, CAP_CON, CAP_EFC1, CAP_CON1))
    src = tmp_path / "layout_check.cpp"
    src.write_text(PROGRAM.replace("@CAPS@", caps).replace("@CHECKS@", "\n".join(checks)))
    exe = tmp_path / "layout_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "mismatches: 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "layouts checked: %d" % len(checks) in out.stdout


def test_spec_header_layout_matches_python_view_of_the_model():
    """The header's dims are the blob's: nq, nv, nu, nbody, ngeom, sum of squared tree sizes, ntree."""
    gen = _generator()
    dims = {name: d for name, _, d in _model_dims()}
    text = open(gen.HEADER).read()
    for struct, model in gen.SPECS:
        block = text[text.index("struct " + struct + " {"):]
        block = block[:block.index("};\n};")]
        assert 'name = "%s";' % model in block
        assert "static constexpr int dims[7] = {%s};" % ", ".join(map(str, dims[model])) in block, (struct, dims[model])
