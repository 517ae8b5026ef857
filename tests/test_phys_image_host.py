"""The table image of the physics kernels (the hot model tables every block copies into LDS), host only, no GPU.

The image's tables and their order are the two lists of csrc/avsim_phys_layout.h (AVSIM_IMG_INT_TABLES, AVSIM_IMG_REAL_TABLES); MOff, Env's
accessors and the check at the end of PhysHost::build come from them, and build fills the image one line per table.  A stand-alone program
(host side compiled with -fsanitize=address,undefined) runs PhysHost::init without a device for every committed model, f32 and f64, and
writes MOff word by word, img_int and img_real.  Here every table is worked out from the model blob alone, in numpy, and compared:

* the tables are contiguous in list order, the first at 0 in each half; nint / nreal are the totals rounded up to four, zero padded;
* each table's words equal the expectation exactly: the pass-through tables are the blob's arrays of the same name, the derived ones are
  recomputed from their definitions (DERIVED below).  geom_cpos alone is compared with an absolute tolerance of 1e-12: values of order 1 m,
  each three double products and three sums, so 1e-12 is far above rounding and far below any wrong table;
* a table that is in a list but has no expectation here fails the test.

The negative case builds the same program against a copy of the physics header with one fill line taken out: init must fail and name the
table."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "av_aloha_amd", "csrc")
MODELS = sorted(glob.glob(os.path.join(ROOT, "models", "*.avm")))

# tables that are the blob's array of the same name (PhysHost::build fills them from I("name") / F("name"))
PASS_THROUGH = {
    "body_parent", "body_jntadr", "body_jntnum", "body_dofadr", "body_dofnum", "body_tree", "tree_dofadr", "tree_dofnum", "jnt_type", "jnt_qposadr",
    "jnt_dofadr", "jnt_actfrclimited", "dof_body", "dof_parent", "dof_tree", "dof_jnt", "act_dof", "act_qposadr", "act_ctrllimited", "geom_type",
    "geom_body",
    "body_pos", "body_quat", "body_mass", "body_ipos", "body_inertia", "body_invweight0", "jnt_pos", "jnt_axis", "jnt_range", "jnt_actfrcrange",
    "jnt_margin", "dof_armature", "dof_damping", "dof_frictionloss", "dof_invweight0", "act_kp", "act_kv", "act_gear", "act_ctrlrange", "geom_rbound",
}


def _lists():
    text = open(os.path.join(CSRC, "avsim_phys_layout.h")).read()
    out = []
    for macro in ("AVSIM_IMG_INT_TABLES", "AVSIM_IMG_REAL_TABLES"):
        m = re.search(r"#define %s\(X\)((?:.*\\\n)*.*)\n" % macro, text)
        body = m.group(1).replace("\\\n", " ")
        names = re.findall(r"X\((\w+)\)", body)
        assert names and not re.sub(r"X\(\w+\)", "", body).strip(), (macro, body)
        out.append(names)
    return out


INT_TABLES, REAL_TABLES = _lists()


def _body_dofmask(a):
    """bit k: dof k of the body's tree lies on the path from the tree's root to the body (the body's own dofs and its ancestors')"""
    parent, tree, adr, num, tadr = a("body_parent"), a("body_tree"), a("body_dofadr"), a("body_dofnum"), a("tree_dofadr")
    mask = np.zeros(len(parent), dtype=np.int64)
    for b in range(1, len(parent)):
        c = b
        while c > 0 and tree[b] >= 0:
            for d in range(adr[c], adr[c] + num[c]):
                mask[b] |= 1 << (d - tadr[tree[b]])
            c = parent[c]
    return mask


def _body_last(a):
    """the last body id of each body's subtree"""
    parent = a("body_parent")
    last = np.arange(len(parent))
    for d in range(len(parent)):
        c = d
        while c > 0:
            c = parent[c]
            last[c] = max(last[c], d)
    return last


def _tree_bodies(a):
    tree = a("body_tree")
    return [np.flatnonzero(tree == t) for t in range(len(a("tree_dofnum")))]


def _ment(a, which):
    """every dof with each of its ancestors, itself first, walking dof_parent"""
    parent, out = a("dof_parent"), []
    for i in range(len(parent)):
        j = i
        while j >= 0:
            out.append((i, j)[which])
            j = parent[j]
    return np.asarray(out, dtype=np.int64)


def _geom_cpos(a):
    q = a("geom_quat").reshape(-1, 4)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    return (a("geom_pos").reshape(-1, 3) + np.einsum("gij,gj->gi", R, a("geom_bcenter").reshape(-1, 3))).reshape(-1)


DERIVED = {
    "body_dofmask": _body_dofmask,
    "body_last": _body_last,
    "tree_bodyadr": lambda a: np.concatenate([[0], np.cumsum([len(t) for t in _tree_bodies(a)])]),
    "tree_bodylist": lambda a: np.concatenate(_tree_bodies(a) + [np.zeros(0, dtype=np.int64)]),
    "tree_madr": lambda a: np.concatenate([[0], np.cumsum(a("tree_dofnum").astype(np.int64) ** 2)])[:-1],
    "limited_jnt": lambda a: np.flatnonzero(a("jnt_limited") != 0),
    "floss_dof": lambda a: np.flatnonzero(a("dof_frictionloss") > 0),
    "ment_i": lambda a: _ment(a, 0),
    "ment_j": lambda a: _ment(a, 1),
    "geom_static": lambda a: (a("body_tree")[a("geom_body")] < 0).astype(np.int64),
    "geom_cpos": _geom_cpos,
}
TOLERANCE = {"geom_cpos": 1e-12}      # absolute; every other table exactly


def _expected(path, name):
    from av_aloha_amd.compiler.compile import read_blob
    md = read_blob(path)
    a = lambda k: np.asarray(md[k]).reshape(-1)
    assert (name in PASS_THROUGH) != (name in DERIVED), "table %s of avsim_phys_layout.h's lists has no expectation in this test (or two)" % name
    return a(name) if name in PASS_THROUGH else np.asarray(DERIVED[name](a))


PROGRAM = r"""
#include <cstdio>
#include <fstream>
#include <iterator>
#define AVSIM_NO_F32_LAUNCH 1      // no kernel is instantiated here
#include "avsim_phys.hip.h"
using namespace avs;
// (the kernels are other units': this program only assembles the image)
namespace avs { const void* phys_spec_kernel(const PhysHost&, const char**) { return nullptr; }
int phys_launch_f64(PhysHost&, hipStream_t, int, const float*, void*, void*, void*, void*, int*, double*, int32_t*, uint8_t*, std::string&) { return -1; } }
// usage: image_dump OUT_DIR model.avm ...: OUT_DIR/<model>.<f32|f64>.bin = MOff's words, img_int, img_real
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        for (int k = 2; k < argc; k++) for (int f64 = 0; f64 < 2; f64++) {
            const std::string path(argv[k]);
            std::ifstream f(path, std::ios::binary);
            const std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            std::string model = path.substr(path.find_last_of('/') + 1);
            model = model.substr(0, model.find_last_of('.'));
            const Blob b(bytes.data(), bytes.size());
            PhysHost ph;
            ph.host_only = true;
            std::string err;
            if (!ph.init(b, 2, f64 != 0, err)) { std::printf("init failed: %s: %s\n", model.c_str(), err.c_str()); return 3; }
            static_assert(sizeof(MOff) == MOFF_WORDS * sizeof(int), "a struct of ints, no padding");
            if ((size_t)ph.moff.nint != ph.img_int.size() || (size_t)ph.moff.nreal != ph.img_real.size()) { std::printf("%s: nint / nreal are not the image's sizes\n", model.c_str()); return 1; }
            std::ofstream o(std::string(argv[1]) + "/" + model + (f64 ? ".f64.bin" : ".f32.bin"), std::ios::binary);
            o.write(reinterpret_cast<const char*>(&ph.moff), sizeof(MOff));
            o.write(reinterpret_cast<const char*>(ph.img_int.data()), ph.img_int.size() * sizeof(int));
            o.write(reinterpret_cast<const char*>(ph.img_real.data()), ph.img_real.size() * sizeof(double));
            if (!o) { std::printf("%s: write failed\n", model.c_str()); return 1; }
        }
    } catch (const std::exception& e) { std::printf("exception: %s\n", e.what()); return 1; }
    std::printf("images written: %d\n", 2 * (argc - 2));
    return 0;
}
"""


def _compile(src_dir, exe):
    """the program, next to whichever avsim_phys.hip.h lies in src_dir (none: the committed one, through -I)"""
    src = src_dir / "image_dump.cpp"
    src.write_text(PROGRAM)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "--offload-arch=gfx950", "-x", "hip",
                           "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = tmp_path_factory.mktemp("phys_image")
    exe = _compile(d, d / "image_dump")
    out = subprocess.run([str(exe), str(d)] + MODELS, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "images written: %d" % (2 * len(MODELS)) in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return d


def test_lists_are_the_image_in_order():
    assert len(INT_TABLES) == 31 and len(REAL_TABLES) == 21 and len(set(INT_TABLES + REAL_TABLES)) == 52
    assert (INT_TABLES[0], INT_TABLES[-1], REAL_TABLES[0], REAL_TABLES[-1]) == ("body_parent", "geom_static", "body_pos", "geom_rbound")
    assert len(MODELS) >= 15


def test_image_of_every_model_equals_the_blobs_tables(images):
    nwords = 2 + len(INT_TABLES) + len(REAL_TABLES)
    for path in MODELS:
        model = os.path.basename(path)[:-4]
        want = {name: _expected(path, name) for name in INT_TABLES + REAL_TABLES}
        for prec in ("f32", "f64"):      # (the host's image is of doubles either way: the upload converts)
            raw = open(os.path.join(str(images), "%s.%s.bin" % (model, prec)), "rb").read()
            moff = np.frombuffer(raw, dtype="<i4", count=nwords)
            nreal, nint = int(moff[0]), int(moff[1])
            assert len(raw) == 4 * nwords + 4 * nint + 8 * nreal, (model, prec)
            img_int = np.frombuffer(raw, dtype="<i4", count=nint, offset=4 * nwords)
            img_real = np.frombuffer(raw, dtype="<f8", count=nreal, offset=4 * nwords + 4 * nint)
            off = dict(zip(INT_TABLES + REAL_TABLES, moff[2:].tolist()))
            for tables, img, total in ((INT_TABLES, img_int, nint), (REAL_TABLES, img_real, nreal)):
                at = 0
                for name in tables:
                    n = len(want[name])
                    assert off[name] == at, (model, prec, name, off[name], at)
                    got = img[at:at + n]
                    assert len(got) == n, (model, prec, name)
                    if name in TOLERANCE:
                        assert np.abs(got - want[name]).max() <= TOLERANCE[name], (model, prec, name)
                    else:
                        assert np.array_equal(got, want[name]), (model, prec, name)
                    at += n
                assert total == (at + 3) // 4 * 4 and not img[at:].any(), (model, prec, total, at)


def test_a_listed_table_that_build_does_not_fill_fails_init(tmp_path):
    """A copy of the physics header without dof_jnt's fill line: PhysHost::build's check names the table instead of leaving offset 0."""
    lines = open(os.path.join(CSRC, "avsim_phys.hip.h")).read().split("\n")
    kept = [ln for ln in lines if not re.match(r"\s*IMG_INT\(dof_jnt,", ln)]
    assert len(kept) == len(lines) - 1
    (tmp_path / "avsim_phys.hip.h").write_text("\n".join(kept))      # (found before the committed one: it lies next to the program)
    exe = _compile(tmp_path, tmp_path / "image_dump_skip")
    out = subprocess.run([str(exe), str(tmp_path), MODELS[0]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 3, out.stdout[-3000:] + out.stderr[-3000:]
    assert re.search(r"init failed: \w+: physics init: table image: dof_jnt ", out.stdout), out.stdout
    assert not glob.glob(str(tmp_path / "*.bin"))
