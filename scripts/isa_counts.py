#!/usr/bin/env python3
"""Static counts over kernels of a gfx950 assembly listing (hipcc -S --cuda-device-only).

usage: isa_counts.py FILE.s [kernel-name regex, default k_light_shade|k_camera_step]

Per kernel: VGPRs, scratch bytes, LDS bytes, global loads and stores by width
(x4 / x3 / x2 / x1 / sub-dword), LDS reads, flat loads, and the vmcnt waits
(how many of them drain the queue: vmcnt(0)).  A kernel whose waits are about
as many as its loads runs its loads one behind the other.
"""
import re
import sys


def kernels(text):
    """(name, body, metadata block) for every kernel of the listing."""
    out = []
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        out.append((name, body))
    return out


def widths(body, op):
    w = {"x4": 0, "x3": 0, "x2": 0, "x1": 0, "sub": 0}
    for m in re.finditer(r"^\s*global_%s_(\w+)" % op, body, re.M):
        k = m.group(1)
        if k.startswith("dwordx4"):
            w["x4"] += 1
        elif k.startswith("dwordx3"):
            w["x3"] += 1
        elif k.startswith("dwordx2"):
            w["x2"] += 1
        elif k.startswith("dword"):
            w["x1"] += 1
        else:
            w["sub"] += 1
    return w


def main():
    path = sys.argv[1]
    rx = re.compile(sys.argv[2] if len(sys.argv) > 2 else r"k_light_shade|k_camera_step")
    text = open(path).read()
    print("kernel | VGPRs | scratch | LDS | global loads (x4/x3/x2/x1/sub) | global stores (x4/x3/x2/x1/sub) | "
          "ds_read | flat_load | s_waitcnt vmcnt (vmcnt(0))")
    for name, body in kernels(text):
        if not rx.search(name):
            continue

        def meta(key):
            m = re.search(r"\.amdhsa_%s\s+(\d+)" % key, body)
            return int(m.group(1)) if m else -1

        vg = re.search(r"; NumVgprs: (\d+)", text[text.index(name + ":"):])
        ld, st = widths(body, "load"), widths(body, "store")
        waits = re.findall(r"^\s*s_waitcnt[^\n]*vmcnt\((\d+)\)", body, re.M)
        fmt = lambda w: "%d (%d/%d/%d/%d/%d)" % (sum(w.values()), w["x4"], w["x3"], w["x2"], w["x1"], w["sub"])
        print(" | ".join([
            name, vg.group(1) if vg else "?", str(meta("private_segment_fixed_size")),
            str(meta("group_segment_fixed_size")), fmt(ld), fmt(st),
            str(len(re.findall(r"^\s*ds_read", body, re.M))), str(len(re.findall(r"^\s*flat_load", body, re.M))),
            "%d (%d)" % (len(waits), sum(1 for x in waits if x == "0"))]))


if __name__ == "__main__":
    main()
