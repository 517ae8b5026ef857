"""Static addressing counts of the physics kernels' device assembly (no GPU needed).

Compiles avsim_phys_spec.hip (the per-model f32 kernels), avsim_api.hip (the generic f32 kernel) and avsim_phys_f64.hip to gfx950
assembly with the flag lists of av_aloha_amd/build.py and prints, per function: instructions, global loads and stores by form (`off`: a
64-bit VGPR address; `saddr`: an SGPR base plus one 32-bit VGPR offset), the address arithmetic (v_ashrrev_i32 .., 31, v_lshl_add_u64,
v_mad_u64_u32 / v_mad_i64_i32), s_load, s_waitcnt with lgkmcnt(0) and with vmcnt(0), v_readlane + v_writelane, scratch loads and stores,
VGPRs and ScratchSize; per kernel the resource remarks (VGPRs, SGPR / VGPR spills, ScratchSize, occupancy).

    python tools/asm_addr_counts.py [--src DIR] [--json OUT.json] [--label NAME] [--all]

--src: the csrc directory to compile (default: this tree's; another revision's checkout gives that revision's table).  Without --all only
the physics functions are listed (k_phys, Env's members, the solver and the narrow-phase functions by name: PHYS below).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from av_aloha_amd.build import COMMON_FLAGS, F32_FLAGS, F64_FLAGS  # noqa: E402

UNITS = [("avsim_phys_spec", F32_FLAGS), ("avsim_api", F32_FLAGS), ("avsim_phys_f64", F64_FLAGS)]
PHYS = re.compile(r"k_phys|3Env|pgs_groups|noslip|qcqp|newton|ndense|narrow|box_box|mpr_|multiccd|load_shape|support")
COLS = ["insts", "g_off", "g_saddr", "ashr31", "lshl_add_u64", "mad64", "s_load", "wait_lgkm0", "wait_vm0", "lane_rw", "scratch_ld", "scratch_st", "vgprs", "scratch_B"]


def compile_unit(src, name, flags, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + [f for f in COMMON_FLAGS if f != "-fPIC"] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                                        "-o", out, os.path.join(src, name + ".hip")]
    return subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)


def demangle(names):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except Exception:
            continue
    return {n: n for n in names}


def short(d):
    """avs::Env<float, 64, avs::SpecX>::collide() -> collide [SpecX]; templates of free functions kept short"""
    spec = re.search(r"Spec(\w+)", d)
    m = re.search(r"Env<[^>]*>::(\w+)", d)
    if m:
        base = m.group(1)
    else:
        base = re.sub(r"^(?:void |int |float |double )?avs::", "", d).split("(")[0]
        base = re.sub(r"avs::|, avs::KFixed<.*| const AS4\*", "", base)
        base = re.sub(r"<(float|double), 64, 8, (false|true).*", lambda q: "<%s%s>" % (q.group(1), ", two-tier" if q.group(2) == "true" else ""), base)
        base = re.sub(r", KArgs<\w+>>?", "", base)
        if base.count("<") > base.count(">"):
            base += ">"
    if "Env<double" in d and m:
        base += " <double>"
    return base[:60] + (" [" + spec.group(1) + "]" if spec else "")


def count_function(lines):
    c = dict.fromkeys(COLS, 0)
    for ln in lines:
        t = ln.strip()
        if not t or t[0] in ".;" or t.endswith(":"):
            continue
        op = t.split()[0]
        if not re.match(r"^[a-z]+_", op):
            continue
        c["insts"] += 1
        if op.startswith("global_load") or op.startswith("global_store") or op.startswith("global_atomic"):
            c["g_off" if re.search(r",\s*off\b", t) else "g_saddr"] += 1
        elif op.startswith("v_ashrrev_i32") and re.search(r",\s*31,", t):
            c["ashr31"] += 1
        elif op.startswith("v_lshl_add_u64"):
            c["lshl_add_u64"] += 1
        elif op.startswith("v_mad_u64_u32") or op.startswith("v_mad_i64_i32"):
            c["mad64"] += 1
        elif op.startswith("s_load"):
            c["s_load"] += 1
        elif op == "s_waitcnt":
            if "lgkmcnt(0)" in t:
                c["wait_lgkm0"] += 1
            if "vmcnt(0)" in t:
                c["wait_vm0"] += 1
        elif op.startswith("v_readlane") or op.startswith("v_writelane"):
            c["lane_rw"] += 1
        elif op.startswith("scratch_load"):
            c["scratch_ld"] += 1
        elif op.startswith("scratch_store"):
            c["scratch_st"] += 1
    return c


def parse_asm(path):
    funcs, order = {}, []
    cur, body = None, []
    text = open(path).read().split("\n")
    i = 0
    while i < len(text):
        ln = text[i]
        m = re.match(r"^\t\.type\t(\S+),@function", ln)
        if m:
            cur, body = m.group(1), []
        elif cur and re.match(r"^\.Lfunc_end\d+:", ln):
            c = count_function(body)
            # the trailer comments: "; NumVgprs: N", "; ScratchSize: N"
            for j in range(i, min(i + 80, len(text))):
                mv = re.match(r"^; NumVgprs: (\d+)", text[j])
                ms = re.match(r"^; ScratchSize: (\d+)", text[j])
                if mv:
                    c["vgprs"] = int(mv.group(1))
                if ms:
                    c["scratch_B"] = int(ms.group(1))
                    break
            funcs[cur] = c
            order.append(cur)
            cur = None
        elif cur:
            body.append(ln)
        i += 1
    return funcs, order


def parse_remarks(log):
    kernels, cur = {}, None
    for ln in log.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", ln)
        if m and cur:
            kernels[cur][m.group(1)] = int(m.group(2))
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "av_aloha_amd", "csrc"))
    ap.add_argument("--json")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--keep", help="directory to keep the .s files in")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="asm_addr_")
    os.makedirs(tmp, exist_ok=True)
    procs = [(n, compile_unit(a.src, n, f, os.path.join(tmp, n + ".s"))) for n, f in UNITS]
    result = {"label": a.label, "units": {}}
    for name, p in procs:
        _, err = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(err)
            raise SystemExit("compiling %s failed" % name)
        funcs, order = parse_asm(os.path.join(tmp, name + ".s"))
        kernels = parse_remarks(err)
        dm = demangle(order + list(kernels))
        rows = {}
        for f in order:
            if a.all or PHYS.search(f):
                rows[short(dm[f])] = funcs[f]
        result["units"][name] = {"functions": rows, "kernels": {short(dm[k]): v for k, v in kernels.items() if a.all or PHYS.search(k)}}
        print("== %s (%s)" % (name, a.label))
        w = max([len(k) for k in rows] + [8])
        print("%-*s " % (w, "function") + " ".join("%12s" % c for c in COLS))
        for k, c in rows.items():
            print("%-*s " % (w, k) + " ".join("%12d" % c[x] for x in COLS))
        tot = {x: sum(c[x] for c in rows.values()) for x in COLS[:-2]}
        print("%-*s " % (w, "(sum)") + " ".join("%12d" % tot[x] for x in COLS[:-2]))
        for k, v in result["units"][name]["kernels"].items():
            print("   kernel %s: %s" % (k, ", ".join("%s %d" % kv for kv in v.items())))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
