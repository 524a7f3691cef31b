"""When the waves of one launch of the affine trajectory kernel finish, SIMD by SIMD (run on the GPU box):

    python tools/wave_finish_times.py [--pace 0|1] [--binary PATH] > profiles/wave_pacing_finish_times_<build>.txt

Builds tools/wave_finish_times.hip (the diagnostic build of csrc/trajectory.hip with a stamp per wave; the shipped kernels hold
none) unless the binary is there, and runs it -- a fresh process per launch, each under its own time limit; the first failure
ends the script -- on the headline shape (Euler, 65536 x 64, 1000 steps: 16 waves per SIMD, 8 resident) and the BASELINE
configs[3] shard (midpoint, 32768 x 64: 8 waves per SIMD, one round), plus each method at the other of the two sizes: two
launches of a method that differ by 8 waves per SIMD give the steady-state cost of a wave, (T_16 - T_8) / 8, with whatever a
launch loses at its start and its end cancelled, and T - waves x cost is then what one launch loses there.

Per shape: a wave's duration; per SIMD (XCC, SE, SH, CU, SIMD of HW_ID) the sorted finish times as fractions of the launch; the
time the SIMD spends with 1, 2, 3, ... resident waves after its last wave has started; and the stop condition of the wave-pacing
work: does the last wave of a SIMD run alone for less than 2 % of one wave's duration?"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TICK_US = 0.01                    # s_memrealtime counts at 100 MHz
POW2_STEPS, PACE_WAVES = 1, 2     # tsde_traj_t.flags (include/torchsde_amd.h)
EULER, MIDPOINT = 0, 3


def build(binary):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-o", binary,
                    os.path.join(HERE, "wave_finish_times.hip")], check=True)


def stamps(binary, rows, d, n_steps, method, flags):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "stamps.bin")
        subprocess.run(["timeout", "-k", "10", "120", binary, str(rows), str(d), str(n_steps), str(method), str(flags), out],
                       check=True, stdout=subprocess.DEVNULL)
        return np.fromfile(out, dtype=np.uint64).reshape(-1, 4)


def simd_of(hw):
    """(XCC, SE, SH, CU, SIMD) as one integer key per wave; HW_ID: simd 5:4, cu 11:8, sh 12, se 15:13; XCC_ID 3:0 above bit 32."""
    lo, xcc = hw & np.uint64(0xFFFFFFFF), (hw >> np.uint64(32)) & np.uint64(0xF)
    simd, cu, sh, se = (lo >> np.uint64(4)) & np.uint64(3), (lo >> np.uint64(8)) & np.uint64(0xF), \
        (lo >> np.uint64(12)) & np.uint64(1), (lo >> np.uint64(13)) & np.uint64(7)
    return ((((xcc * np.uint64(8) + se) * np.uint64(2) + sh) * np.uint64(16) + cu) * np.uint64(4) + simd).astype(np.int64)


def key_name(key):
    simd, key = key % 4, key // 4
    cu, key = key % 16, key // 16
    sh, key = key % 2, key // 2
    return f"xcc{key // 8} se{key % 8} sh{sh} cu{cu:<2d} simd{simd}"


def residency_tail(start, end):
    """Seconds-free: ticks a SIMD spends with r = 1, 2, ... resident waves after its last wave has started."""
    t_last_start = start.max()
    ends = np.sort(end[end > t_last_start])
    edges = np.concatenate(([t_last_start], ends))
    resident = len(ends) - np.arange(len(ends))            # waves resident during edges[i] .. edges[i + 1]
    return {int(r): float(edges[i + 1] - edges[i]) for i, r in enumerate(resident)}


def report(name, s):
    start, end, key = s[:, 0].astype(np.float64), s[:, 1].astype(np.float64), simd_of(s[:, 2])
    t0 = start.min()
    launch = end.max() - t0
    dur = end - start
    simds = np.unique(key)
    per = [np.flatnonzero(key == k) for k in simds]
    counts = np.array([len(ix) for ix in per])
    print(f"== {name}: {len(s)} waves on {len(simds)} SIMDs ({counts.min()}..{counts.max()} per SIMD, median "
          f"{int(np.median(counts))}); launch (first start to last end) {launch * TICK_US:.1f} us")
    print(f"   a wave's duration: min {dur.min() * TICK_US:.1f}  median {np.median(dur) * TICK_US:.1f}  max "
          f"{dur.max() * TICK_US:.1f} us   ({np.median(dur) / launch:.3f} of the launch)")
    print(f"   resident waves per SIMD, mean over the launch (sum of durations / SIMDs / launch): "
          f"{dur.sum() / len(simds) / launch:.2f}   (what SQ_WAVE_CYCLES x 4 / SIMDs / (GRBM_GUI_ACTIVE / 8) gives if the "
          f"counter is in quad-cycles)")
    simd_end = np.array([end[ix].max() for ix in per])
    print(f"   a SIMD's last wave ends at: min {(simd_end.min() - t0) / launch:.4f}  median "
          f"{(np.median(simd_end) - t0) / launch:.4f}  max 1.0000 of the launch")
    m = int(np.median(counts))
    full = [ix for ix in per if len(ix) == m]
    fin = np.array([np.sort(end[ix] - t0) / launch for ix in full])            # (SIMDs with m waves, m)
    print(f"   sorted finish times of a SIMD's waves as fractions of the launch, over the {len(full)} SIMDs with {m} waves:")
    print("     rank    " + " ".join(f"{i + 1:>6d}" for i in range(m)))
    for label, row in (("min", fin.min(0)), ("median", np.median(fin, 0)), ("max", fin.max(0))):
        print(f"     {label:<7s} " + " ".join(f"{v:6.3f}" for v in row))
    print("   the first 8 SIMDs in full:")
    for k, ix in list(zip(simds, per))[:8]:
        print(f"     {key_name(int(k))}: " + " ".join(f"{v:.3f}" for v in np.sort(end[ix] - t0) / launch))
    tails = [residency_tail(start[ix], end[ix]) for ix in per]
    wave = np.median(dur)
    print("   time a SIMD spends with r resident waves after its last wave has started, in units of the median wave duration "
          "(median over SIMDs; mean; max):")
    for r in range(1, max(max(t) for t in tails) + 1):
        v = np.array([t.get(r, 0.0) for t in tails]) / wave
        print(f"     r = {r}: {np.median(v):7.4f}  {v.mean():7.4f}  {v.max():7.4f}")
    alone = np.array([t.get(1, 0.0) for t in tails]) / wave
    print(f"   the last wave of a SIMD runs alone for {np.median(alone) * 100:.2f} % of one wave's duration (median over SIMDs; "
          f"mean {alone.mean() * 100:.2f} %, max {alone.max() * 100:.2f} %); below 2 % there is no tail: "
          f"{'NO TAIL' if np.median(alone) < 0.02 and alone.mean() < 0.02 else 'a tail'}")
    return launch * TICK_US, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pace", type=int, default=1, help="TSDE_TRAJ_PACE_WAVES in the launches' flags (0: the unpaced loop)")
    ap.add_argument("--binary", default=os.path.join(HERE, "wave_finish_times"))
    ap.add_argument("--steps", type=int, default=1000)
    args = ap.parse_args()
    if not os.path.exists(args.binary):
        build(args.binary)
    flags = POW2_STEPS | (PACE_WAVES if args.pace else 0)
    print(f"tools/wave_finish_times.py: flags {flags} (pow2 steps{', paced waves' if args.pace else ''}), {args.steps} steps, d = 64; "
          "times from s_memrealtime (100 MHz)")
    t = {}
    for method, label in ((EULER, "Euler"), (MIDPOINT, "midpoint")):
        for rows in (65536, 32768):
            name = f"{label} {rows} x 64" + {(EULER, 65536): " (the headline shape)",
                                             (MIDPOINT, 32768): " (the configs[3] shard shape)"}.get((method, rows), "")
            t[method, rows] = report(name, stamps(args.binary, rows, 64, args.steps, method, flags))
            sys.stdout.flush()
    print("== what a launch loses at its start and end: T - waves x cost, cost = (T_65536 - T_32768) / (difference in waves per SIMD)")
    for method, label in ((EULER, "Euler"), (MIDPOINT, "midpoint")):
        (t_hi, m_hi), (t_lo, m_lo) = t[method, 65536], t[method, 32768]
        cost = (t_hi - t_lo) / (m_hi - m_lo)
        for rows, (tt, m) in ((65536, (t_hi, m_hi)), (32768, (t_lo, m_lo))):
            print(f"   {label} {rows} x 64: {tt:.1f} us = {m} waves x {cost:.2f} us + {tt - m * cost:.1f} us "
                  f"({(tt - m * cost) / tt * 100:.2f} % of the launch, {(tt - m * cost) / cost:.3f} of one wave's steady-state cost)")


if __name__ == "__main__":
    main()
