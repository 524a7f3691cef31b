"""Turn the remarks of ``hipcc -Rpass-analysis=kernel-resource-usage`` (read from stdin or a file) into one line per kernel:

    neural_trajectory_kernel<D, H, MODE, SPLIT, GENERIC[, MILSTEIN]>  sgpr vgpr agpr scratch occupancy sgpr_spill vgpr_spill lds

so that two builds of csrc/mlp_general.hip can be compared with `diff` (a defaulted trailing template argument is printed as the
build mangles it: the comparison keys on the first five)."""
import re
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def kernel_name(mangled):
    m = re.search(r"neural_trajectory_kernelI((?:L[ib]\d+E)+)E", mangled)
    if not m:
        return mangled
    args = [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))]
    args += [0] * (6 - len(args))
    D, H, mode, split, generic, milstein = args[:6]
    noise = {0: "diagonal", 1: "scalar", 2: "additive"}.get(mode, f"general m={mode}")
    flags = "".join(f", {name}" for name, on in (("split-bf16", split), ("element-wise rows", generic), ("MILSTEIN", milstein)) if on)
    return f"neural_trajectory_kernel<D={D}, H={H}, {noise}{flags}>"


def listing(text):
    rows, current = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            current = {"name": kernel_name(m.group(1))}
            rows.append(current)
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and current is not None:
            current[m.group(1).strip()] = m.group(2)
    out = [f"{'kernel':<78} " + " ".join(f"{h:>9}" for h in ("sgpr", "vgpr", "agpr", "scratch", "occupancy", "sgpr_spill",
                                                              "vgpr_spill", "lds"))]
    for r in sorted(rows, key=lambda r: r["name"]):
        out.append(f"{r['name']:<78} " + " ".join(f"{r.get(f, '?'):>9}" for f in FIELDS))
    return "\n".join(out)


if __name__ == "__main__":
    print(listing(open(sys.argv[1]).read() if len(sys.argv) > 1 else sys.stdin.read()))
