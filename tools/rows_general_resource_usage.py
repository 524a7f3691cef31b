"""The size rule of the row kernel with a diffusion matrix (specialise.ROWS_GENERAL_CAP), measured with the compiler.

For each scheme (Euler, midpoint, Heun, Euler-Heun) and each dtype: the generated unit (specialise.source_rows_general) of the
DENSE worst case of every d = 1 .. 8 channels and m = 1 .. 8 Brownian channels -- every drift channel and every entry of the
diffusion matrix reads every state channel, a constant of its own and t (tests/helpers_rows_general.DenseWorst) -- compiled for
gfx950 with -Rpass-analysis=kernel-resource-usage. The cap of a scheme and dtype on d * m lies below the first (d, m) whose unit
has scratch or spilled vector registers (64 = every pair fits); every figure is written down.

    python tools/rows_general_resource_usage.py [--out profiles/rows_general_resource_usage.txt] [--jobs 8]

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
from tests.helpers_rows_general import DenseWorst  # noqa: E402
from torchsde_amd import _native, recognise_rows, specialise  # noqa: E402
from torchsde_amd.sde import ForwardSDE  # noqa: E402

SCHEMES = {"euler": _native.TRAJ_EULER, "midpoint": _native.TRAJ_MIDPOINT, "heun": _native.TRAJ_HEUN,
           "euler_heun": _native.TRAJ_EULER_HEUN}
FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill", "SGPRs Spill")
DTYPES = {"float32": torch.float32, "float64": torch.float64}


def dense_structure(d, m):
    """(structure, number of constants) of the dense worst case, through the interpreter the solves use."""
    found = recognise_rows.recognise_rows(ForwardSDE(DenseWorst(d, m)), torch.tensor(0.3), torch.rand(7, d), m=m)
    assert not any(found.zero_mask)
    return found.structure(), len(found.consts)


def resource_usage(structure, n_const, method, dtype):
    """{field: value} of the compiled unit's kernel."""
    text = specialise.source_rows_general(structure, n_const, dtype, method)
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "unit.hip"), os.path.join(tmp, "unit.so")
        with open(src, "w") as fh:
            fh.write(text)
        done = subprocess.run(specialise._compile_command("gfx950", out, src) + ["-Rpass-analysis=kernel-resource-usage"],
                              capture_output=True, text=True, timeout=1800)
    if done.returncode != 0:
        raise RuntimeError(done.stderr[-2000:])
    return {field: int(re.search(re.escape(field) + r": (\d+)", done.stderr).group(1)) for field in FIELDS}


def fits(usage):
    return usage["ScratchSize [bytes/lane]"] == 0 and usage["VGPRs Spill"] == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    pairs = [(d, m) for d in range(1, recognise_rows.MAX_D + 1) for m in range(1, recognise_rows.MAX_M + 1)]
    structures = {pair: dense_structure(*pair) for pair in pairs}
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        jobs = {(name, d, m, dname): pool.submit(resource_usage, *structures[(d, m)], SCHEMES[name], DTYPES[dname])
                for name in SCHEMES for d, m in pairs for dname in DTYPES}
        table = {key: job.result() for key, job in jobs.items()}
    caps = {}
    for name in SCHEMES:
        for dname in DTYPES:
            over = [d * m for d, m in pairs if not fits(table[(name, d, m, dname)])]
            caps[(name, dname)] = min(over) - 1 if over else recognise_rows.MAX_D * recognise_rows.MAX_M
    lines = ["# the dense worst case's unit of the row kernel with a diffusion matrix, gfx950 (tools/rows_general_resource_usage.py):",
             "# every d = 1 .. 8, m = 1 .. 8; a scheme's cap on d*m lies below the first (d, m) with scratch or spilled vector",
             "# registers (64: every pair fits)",
             "# scheme d m d*m dtype : " + ", ".join(FIELDS)]
    for name in SCHEMES:
        lines.append(f"## {name}: cap d*m = " + ", ".join(f"{caps[(name, dname)]} ({dname})" for dname in DTYPES))
        for dname in DTYPES:
            for d, m in pairs:
                usage = table[(name, d, m, dname)]
                lines.append(f"{name} {d} {m} {d * m} {dname} : " + ", ".join(f"{f} {usage[f]}" for f in FIELDS)
                             + ("" if fits(usage) else "   <- over"))
    print("\n".join(line for line in lines if line.startswith("#")))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
