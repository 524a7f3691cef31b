"""The size rule of the row-coupled tangent kernel (specialise.ROWS_SENS_CAP), measured with the compiler.

For each scheme: the generated tangent unit (specialise.source_rows_sens) of a DENSE synthetic system -- every drift and every
diffusion channel reads every state channel and a trainable constant (tests/helpers_rows_grad.dense_system) -- in float32 and
in float64 (twice the registers per number), compiled for gfx950 with -Rpass-analysis=kernel-resource-usage: d = 8 channels at
NT = 1 .. 16 tangents, then d = 2 .. 7 at every NT the d = 8 figures would admit. The cap of a scheme and dtype is the largest
d * (NT + 1) below the first unit of any d that has scratch or spilled vector registers; every figure is written down.

    python tools/rows_sens_resource_usage.py [--out profiles/rows_sens_resource_usage.txt] [--jobs 8] [--known earlier listing]

Needs hipcc; no GPU.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests.helpers_rows_grad import dense_system  # noqa: E402
from torchsde_amd import _native, specialise  # noqa: E402

SCHEMES = {"euler": _native.TRAJ_EULER, "midpoint": _native.TRAJ_MIDPOINT, "heun": _native.TRAJ_HEUN,
           "euler_heun": _native.TRAJ_EULER_HEUN, "srk": _native.TRAJ_SRK}
FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill", "SGPRs Spill")


def resource_usage(d, nt, method, dtype):
    """{field: value} of the compiled unit's kernel."""
    structure, n_const, slots, y0_grad = dense_system(d, nt)
    text = specialise.source_rows_sens(structure, n_const, dtype, method, slots, y0_grad)
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "unit.hip"), os.path.join(tmp, "unit.so")
        with open(src, "w") as fh:
            fh.write(text)
        done = subprocess.run(specialise._compile_command("gfx950", out, src) + ["-Rpass-analysis=kernel-resource-usage"],
                              capture_output=True, text=True, timeout=1800)
    if done.returncode != 0:
        raise RuntimeError(done.stderr[-2000:])
    found = {}
    for field in FIELDS:
        m = re.search(re.escape(field) + r": (\d+)", done.stderr)
        found[field] = int(m.group(1))
    return found


def fits(usage):
    return usage["ScratchSize [bytes/lane]"] == 0 and usage["VGPRs Spill"] == 0


def known_rows(path):
    """{(scheme, d, NT, dtype): usage} of an earlier listing: units already compiled are not compiled again."""
    table = {}
    if path and os.path.exists(path):
        for line in open(path):
            m = re.match(r"(\w+) (\d+) (\d+) \d+ (float\d+) : (.*?)(   <- over)?$", line.rstrip("\n"))
            if m:
                usage = {f: int(re.search(re.escape(f) + r" (\d+)", m.group(5)).group(1)) for f in FIELDS}
                table[(m.group(1), int(m.group(2)), int(m.group(3)), m.group(4))] = usage
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--known", default=None, help="an earlier listing whose rows are taken over")
    args = ap.parse_args()
    dtypes = {"float32": torch.float32, "float64": torch.float64}
    top = specialise.ROWS_SENS_MAX_TANGENTS
    table = known_rows(args.known)

    def compile_missing(pool, keys):
        jobs = {key: pool.submit(resource_usage, key[1], key[2], SCHEMES[key[0]], dtypes[key[3]]) for key in keys
                if key not in table}
        table.update({key: job.result() for key, job in jobs.items()})

    def first_failure(name, d, dname, upto):
        """The smallest NT <= upto whose unit does not fit, or None."""
        for nt in range(1, upto + 1):
            if not fits(table[(name, d, nt, dname)]):
                return nt
        return None
    caps, limited_by = {}, {}
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        # d = 8, every NT: the widest rows set the starting cap ...
        compile_missing(pool, [(name, 8, nt, dname) for name in SCHEMES for nt in range(1, top + 1) for dname in dtypes])
        for name in SCHEMES:
            for dname in dtypes:
                bad = first_failure(name, 8, dname, top)
                caps[(name, dname)] = 8 * ((bad or top + 1) - 1 + 1) if bad != 1 else 0
                limited_by[(name, dname)] = 8
        # ... and every narrower row, every NT that cap would admit, may only lower it
        admitted = {(name, d, dname): min(top, caps[(name, dname)] // d - 1)
                    for name in SCHEMES for dname in dtypes for d in range(2, 8)}
        compile_missing(pool, [(name, d, nt, dname) for (name, d, dname), upto in admitted.items() for nt in range(1, upto + 1)])
        for (name, d, dname), upto in admitted.items():
            bad = first_failure(name, d, dname, upto)
            if bad is not None and d * (bad + 1) - 1 < caps[(name, dname)]:
                caps[(name, dname)] = d * (bad + 1) - 1
                limited_by[(name, dname)] = d
    lines = ["# the dense synthetic system's tangent unit, gfx950 (tools/rows_sens_resource_usage.py): d = 8 at every NT <= 16, and",
             "# d = 2 .. 7 at every NT the d = 8 cap would admit; a scheme's cap on d*(NT+1) lies below the first unit of ANY d",
             "# that has scratch or spilled vector registers (rows past a d's first failure are not admitted and may fit or not)",
             "# scheme d NT d*(NT+1) dtype : " + ", ".join(FIELDS)]
    for name in SCHEMES:
        lines.append(f"## {name}: cap d*(NT+1) = " + ", ".join(f"{caps[(name, dname)]} ({dname}, set at d = {limited_by[(name, dname)]})"
                                                               for dname in dtypes))
        for key in sorted((k for k in table if k[0] == name), key=lambda k: (k[3], -k[1], k[2])):
            _, dd, nt, dtype = key
            usage = table[key]
            lines.append(f"{name} {dd} {nt} {dd * (nt + 1)} {dtype} : " + ", ".join(f"{f} {usage[f]}" for f in FIELDS)
                         + ("" if fits(usage) else "   <- over"))
    text = "\n".join(lines) + "\n"
    print("\n".join(l for l in lines if l.startswith("#")))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
