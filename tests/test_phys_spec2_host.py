"""Host side of stage two of the per-model physics kernels (dims and solver configuration as constants), no GPU:

* every integer dim that csrc/avsim_phys_specs.h bakes into a kernel equals the model blob's, worked out here from the blob alone;
* every baked solver flag equals what a default f32 handle of that model holds after PhysHost::init, and the launch-time predicate
  (spec_matches) follows the options: a stand-alone program runs init without a device -- the generator's way -- compares the handle's
  integers with the spec's one by one, then sets each solver option off its default and back and asks spec_matches each time.  Its host
  side is compiled with -fsanitize=address,undefined."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "av_aloha_amd", "csrc")
SPECS = {"SpecSlotInsertion3Arms": "slot_insertion_3arms", "SpecHookPackage2Arms": "hook_package_2arms"}
DIMS = ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "npair", "ntree", "neq", "nfloss", "nlimited", "nment", "nj", "msize", "nobj", "task_id", "hull_ovf")
FLAGS = ("solver", "newton_iters", "noslip_iters", "noslip_trees", "noslip_per_tree", "qcqp_tridiag", "newton_early_exit", "newton_component", "ls_iterations")


def _baked(struct):
    text = open(os.path.join(CSRC, "avsim_phys_specs.h")).read()
    block = text[text.index("struct " + struct + " {"):]
    block = block[:block.index("static constexpr Layout lay")]
    decl = block[block.index("static constexpr int nq"):]
    return {k: int(v) for k, v in re.findall(r"(\w+) = (-?\d+)", decl)}


def test_baked_dims_equal_the_model_blob():
    from av_aloha_amd.compiler.compile import read_blob
    for struct, model in SPECS.items():
        md = read_blob(os.path.join(ROOT, "models", model + ".avm"))
        s = lambda k: int(np.asarray(md[k]).reshape(-1)[0])
        a = lambda k: np.asarray(md[k]).reshape(-1)
        parent = a("dof_parent").astype(int)
        depth = np.zeros(len(parent), dtype=int)
        for i, p in enumerate(parent):      # (a dof's parent precedes it)
            depth[i] = 1 + (depth[p] if p >= 0 else 0)
        want = {k: s(k) for k in ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "npair", "ntree", "neq", "task_id")}
        want.update(nfloss=int((a("dof_frictionloss") > 0).sum()), nlimited=int((a("jnt_limited") != 0).sum()), nment=int(depth.sum()),
                    nj=21 if s("num_arms") == 3 else 14, msize=int((a("tree_dofnum").astype(np.int64) ** 2).sum()), nobj=len(a("objects_qposadr")),
                    hull_ovf=8 * len(a("chull_cells")))
        got = _baked(struct)
        assert set(DIMS) | set(FLAGS) == set(got), (struct, sorted(got))
        for k in DIMS:
            assert got[k] == want[k], (struct, k, got[k], want[k])
        assert len(a("pair_geom")) == 2 * got["npair"] and len(a("tree_dofnum")) == got["ntree"]


PROGRAM = r"""
#include <cstdio>
#include <fstream>
#include <iterator>
#define AVSIM_NO_F32_LAUNCH 1      // no kernel is instantiated here
#include "avsim_phys.hip.h"
#include "avsim_phys_specs.h"
using namespace avs;
static int bad = 0, seen = 0;
#define EXPECT(c, ...) do { seen++; if (!(c)) { bad++; std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)
template <typename SPEC> static void check(const std::string& dir) {
    const std::string path = dir + "/" + SPEC::name + ".avm";
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const Blob b(bytes.data(), bytes.size());
    PhysHost ph;
    ph.host_only = true;
    std::string err;
    EXPECT(ph.init(b, 1, false, err), "%s: init: %s", SPEC::name, err.c_str());
#define ONE(x) EXPECT(ph.mf.x == SPEC::x, "%s: " #x " handle %d, spec %d", SPEC::name, ph.mf.x, SPEC::x);
    AVSIM_HEAD_INTS(ONE)
    AVSIM_BODY_INTS(ONE)
#undef ONE
    EXPECT(spec_matches<SPEC>(ph), "%s: a default handle does not match its spec", SPEC::name);
    EXPECT(!ph.refuses(err), "%s: refuses under the default", SPEC::name);
    const struct { const char* name; double off, dflt; } opts[] = {@OPTIONS@};
    for (const auto& o : opts) {
        EXPECT(ph.set_option(o.name, o.off), "%s: set_option(%s)", SPEC::name, o.name);
        EXPECT(!spec_matches<SPEC>(ph), "%s: %s = %g still matches", SPEC::name, o.name, o.off);
        EXPECT(ph.set_option(o.name, o.dflt), "%s: set_option(%s)", SPEC::name, o.name);
        EXPECT(spec_matches<SPEC>(ph), "%s: %s back at %g does not match", SPEC::name, o.name, o.dflt);
    }
    // real-valued options are not compiled in: they do not decide
    EXPECT(ph.set_option("newton_tol", 1e-5) && ph.set_option("ls_tolerance", 1e-3) && spec_matches<SPEC>(ph), "%s: a tolerance changed the match", SPEC::name);
}
// (the kernels are another unit's: this program only asks the predicate)
namespace avs { const void* phys_spec_kernel(const PhysHost&, const char**) { return nullptr; }
int phys_launch_f64(PhysHost&, hipStream_t, int, const float*, void*, void*, void*, void*, int*, double*, int32_t*, uint8_t*, std::string&) { return -1; } }
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
#define RUN(S) check<S>(argv[1]);
        AVSIM_PHYS_SPECS(RUN)
    } catch (const std::exception& e) { std::printf("exception: %s\n", e.what()); return 1; }
    std::printf("checked: %d, mismatches: %d\n", seen, bad);
    return bad ? 1 : 0;
}
"""
# option, a value off the default of an f32 handle, that default
OPTIONS = [("solver", 0, 1), ("newton_iters", 50, 100), ("noslip_iters", 5, 3), ("noslip_trees", 0, 1), ("noslip_per_tree", 0, 1), ("qcqp_tridiag", 0, 2),
           ("newton_early_exit", 0, 1), ("newton_component", 0, 1), ("ls_iterations", 20, 50)]


def test_baked_solver_flags_are_a_default_handles_and_options_decide_the_match(tmp_path):
    assert {o[0] for o in OPTIONS} == set(FLAGS)
    for struct in SPECS:
        got = _baked(struct)
        for name, _, default in OPTIONS:
            assert got[name] == default, (struct, name, got[name])
    src = tmp_path / "spec2_check.cpp"
    src.write_text(PROGRAM.replace("@OPTIONS@", ", ".join('{"%s", %d, %d}' % o for o in OPTIONS)))
    exe = tmp_path / "spec2_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "--offload-arch=gfx950", "-x", "hip",
                           "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), os.path.join(ROOT, "models")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "mismatches: 0" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    per_spec = 26 + 3 + 4 * len(OPTIONS) + 1
    assert "checked: %d," % (len(SPECS) * per_spec) in out.stdout, out.stdout
