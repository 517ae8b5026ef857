"""Regenerates av_aloha_amd/csrc/avsim_phys_specs.h: builds tools/gen_phys_specs.cpp for the host (it includes the physics header and
runs PhysHost::init without a device) and runs it on the models that get a k_phys compiled for them.

    python tools/gen_phys_specs.py            # rewrites the committed header
    python tools/gen_phys_specs.py --out X.h  # writes elsewhere (tests/test_phys_spec_host.py compares that with the committed one)

To give another one-pass model a specialised kernel: add it to SPECS below, run this, and rebuild (avsim_phys_spec.hip instantiates
one kernel per entry of the header's AVSIM_PHYS_SPECS list)."""
import argparse
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "av_aloha_amd", "csrc")
HEADER = os.path.join(CSRC, "avsim_phys_specs.h")
# spec struct -> model (models/<name>.avm)
SPECS = [("SpecSlotInsertion3Arms", "slot_insertion_3arms"), ("SpecHookPackage2Arms", "hook_package_2arms")]


def generate(out, workdir, sanitize=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = os.path.join(workdir, "gen_phys_specs")
    # (the header's two plain kernels want a device image to register: compiled along, never run)
    cmd = [hipcc, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "gen_phys_specs.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd)
    args = ["%s=%s" % (s, os.path.join(ROOT, "models", m + ".avm")) for s, m in SPECS]
    text = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    with open(out, "w") as f:
        f.write(text)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HEADER)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        print(generate(a.out, d))
