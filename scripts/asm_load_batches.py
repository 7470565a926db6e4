#!/usr/bin/env python
"""How many global loads a kernel issues ahead of each counted wait: for every loop of one kernel
in a `hipcc -S` dump, the loads before the first `s_waitcnt vmcnt`, the sequence of vmcnt values,
and the fp64 / fp32 adds and fused multiply-adds of the body.  A load-wait-add loop prints
`loads ahead 1, vmcnt [0]`; a batched ordered sum of depth D prints `loads ahead D, vmcnt [D-1..0]`.
usage: asm_load_batches.py lib.s <mangled-name-substring> [...]"""
import re
import sys

src = open(sys.argv[1]).read().split("\n")
for name in sys.argv[2:]:
    start = next(i for i, l in enumerate(src) if re.match(r"^_Z\w+:", l) and name in l)
    end = next(i for i in range(start, len(src)) if src[i].startswith(".Lfunc_end"))
    lines = src[start:end]
    cnt = lambda pat, body: sum(bool(re.search(pat, x)) for x in body)
    print("%s: %d lines, %d global loads, scratch ops %d, fp64 fma %d" % (
        lines[0].split(":")[0], len(lines), cnt(r"global_load", lines), cnt(r"scratch_", lines), cnt(r"v_fmac?_f64", lines)))
    for hh in [i for i, l in enumerate(lines) if "Loop Header" in l]:
        lab = lines[hh].split(":")[0]
        e = next((j for j in range(hh, len(lines)) if re.search(r"s_c?branch\w* " + re.escape(lab) + r"\b", lines[j])), None)
        if e is None:
            continue
        body = lines[hh:e + 1]
        if not cnt(r"global_load", body):
            continue
        first_wait = next((k for k, x in enumerate(body) if re.search(r"s_waitcnt.*vmcnt", x)), len(body))
        waits = [int(m.group(1)) for x in body for m in [re.search(r"vmcnt\((\d+)\)", x)] if m]
        print("  %-10s %4d lines: loads %2d, loads ahead of the first wait %2d, vmcnt %s, add_f64 %d fma_f64 %d add_f32 %d" % (
            lab, len(body), cnt(r"global_load", body), cnt(r"global_load", body[:first_wait]), waits,
            cnt(r"v_add_f64", body), cnt(r"v_fmac?_f64", body), cnt(r"v_add_f32", body)))
