"""Build check (csrc/Makefile) for every kernel that issues LDS-DMA (lds_dma.h): no scratch and no SGPR spills.

Reads the compiler's -Rpass-analysis=kernel-resource-usage remarks (a text file) and fails if any kernel whose
name contains NAME reports `ScratchSize [bytes/lane]` != 0 or `SGPRs Spill` != 0, or if fewer than COUNT such
kernels are found (a renamed kernel must not pass by not being looked at).

    python3 usage_check.py build/xenc.usage.txt k_xenc_chain 5
"""
import re
import sys


def parse(text):
    """[(function name, {field: int})] in the order of the remarks."""
    kernels = []
    for line in text.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            kernels.append((body.split(":", 1)[1].strip(), {}))
        elif kernels and ":" in body:
            key, val = body.rsplit(":", 1)
            if re.fullmatch(r"\s*-?\d+", val):
                kernels[-1][1][key.strip()] = int(val)
    return kernels


def other_diagnostics(text):
    """The compiler's output without the remarks and the source lines quoted under them (warnings must stay visible)."""
    out, quoted = [], False
    for line in text.splitlines():
        if "remark:" in line:
            quoted = True
        elif quoted and re.match(r"\s*\d*\s*\|", line):
            pass
        else:
            quoted = False
            out.append(line)
    return out


def main(argv):
    path, name, count = argv[1], argv[2], int(argv[3])
    with open(path) as f:
        text = f.read()
    for line in other_diagnostics(text):
        print(line, file=sys.stderr)
    kernels = [(n, u) for n, u in parse(text) if name in n]
    bad = []
    for n, u in kernels:
        scratch = u.get("ScratchSize [bytes/lane]")
        sspill = u.get("SGPRs Spill")
        print(f"{n}: VGPRs {u.get('VGPRs')} AGPRs {u.get('AGPRs')} SGPRs {u.get('TotalSGPRs')} "
              f"scratch {scratch} B/lane, SGPR spills {sspill}, VGPR spills {u.get('VGPRs Spill')}")
        if scratch != 0 or sspill != 0:
            bad.append(n)
    if len(kernels) < count:
        print(f"error: {path}: {len(kernels)} kernels named *{name}* reported, expected {count}", file=sys.stderr)
        return 1
    if bad:
        print(f"error: {name}: scratch memory or SGPR spills in {len(bad)} instantiation(s) (see above and {path}).\n"
              "  These kernels issue LDS-DMA from scalar operands and count its waits by hand (lds_dma.h): a spilled\n"
              "  SGPR next to those operands is unsafe, and every scratch reload drains the queue (vmcnt(0)).\n"
              "  Shorten live ranges until the compiler reports 0 for both.", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
