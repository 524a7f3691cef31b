"""Compare the device assembly of two builds of a translation unit kernel by kernel, keyed on the mangled symbol:

    python tools/kernel_asm_compare.py parent/steps.s new/steps.s [parent/rheun.s new/rheun.s ...]

where each file comes from `hipcc <the Makefile's flags> --cuda-device-only -S`. A body is what stands between `<symbol>:` and
its `.Lfunc_end`. Comments are dropped and the numbers that count functions and long branches within a file (`.LBB12_3`,
`.Lpost_getpc6`) are blanked, so that the order in which templates are instantiated may move and instructions may not. Exits
non-zero if a symbol is missing on either side or a body differs."""
import re
import sys


def bodies(path):
    out, current, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and current is None:
            name, current = m.group(1), []
        elif current is not None:
            if line.startswith(".Lfunc_end"):
                out[name], current = "".join(current), None
            else:
                line = re.sub(r"\s*;.*$", "", line.rstrip("\n"))
                current.append(re.sub(r"(BB|tmp|post_getpc)\d+", r"\1N", line) + "\n")
    return out


def main(paths):
    bad = 0
    for parent, new in zip(paths[0::2], paths[1::2]):
        a, b = bodies(parent), bodies(new)
        missing = sorted(set(a) ^ set(b))
        differ = sorted(k for k in a if k in b and a[k] != b[k])
        print(f"{new}: {len(b)} device functions, {len(missing)} not on both sides, {len(differ)} bodies differ")
        for k in missing + differ:
            print("   ", k)
        bad += len(missing) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
