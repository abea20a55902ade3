#!/usr/bin/env python3
"""Instruction mix per kernel of a gfx950 assembly listing (hipcc -S --cuda-device-only).

  isa_mix.py <listing.s> [name ...]                  one line per function, the 18 commonest opcodes of the named ones
  isa_mix.py --slots <listing.s> [kernel] [--json]   issue slots of a kernel's hot loop (default k_msm_comb30)
  isa_mix.py --spans <listing.s> [kernel]            every backward-branch span of the kernel, one JSON line each, shortest first

--slots takes the kernel's longest backward-branch span (the label a branch jumps back to .. that branch) and counts, for the
span and for its fast-addition block (the first product's opening multiply-add .. the last multiply-add before the span's first
out-of-line call or, without one, its end): VALU instructions, s_nop, the rest, their sum = the issue slots a wave spends
there, and the code bytes (4 per instruction in a 32-bit encoding, 8 for VOP3 / VOP3P / memory / a 32-bit literal)."""
import collections
import json
import re
import sys


def main(path, detail=()):
    s = open(path).read()
    for name in re.findall(r"^(_Z\w+):", s, flags=re.M):
        a = s.index("\n" + name + ":")
        b = s.find(".Lfunc_end", a)  # closes kernels and device functions alike
        body = s[a:b if b > 0 else len(s)]
        ins = []
        for l in body.split("\n"):
            t = l.strip()
            if not l.startswith("\t") or not t or t[0] in ".;":
                continue
            ins.append(t.split()[0])
        c = collections.Counter(ins)
        scratch = sum(v for k, v in c.items() if "scratch" in k)
        print("%-60s %6d instr  mad_u64 %5d  scratch %4d  s_nop %4d" % (name[:60], len(ins), c["v_mad_u64_u32"], scratch, c["s_nop"]))
        if any(d in name for d in detail):
            print("    ", c.most_common(18))


def _instructions(body):
    """(line index, mnemonic, operand text) of every instruction line, and {label: line index}"""
    ins, labels = [], {}
    for n, l in enumerate(body.split("\n")):
        m = re.match(r"^(\.?\w+):", l)
        if m:
            labels[m.group(1)] = n
            continue
        t = l.strip()
        if not l.startswith("\t") or not t or t[0] in ".;":
            continue
        parts = t.split(None, 1)
        ins.append((n, parts[0], parts[1] if len(parts) > 1 else ""))
    return ins, labels


def _bytes(op, args):
    if op.startswith(("s_nop", "s_waitcnt", "s_branch", "s_cbranch", "s_endpgm", "s_sleep", "s_setprio", "s_barrier")):
        return 4
    if op.startswith(("global_", "flat_", "scratch_", "buffer_", "ds_", "s_load", "s_buffer_load")):
        return 8
    lit = 4 if re.search(r"(?<![\w\[])(0x[0-9a-f]{3,}|\d{3,})(?![\w\]:])", args) else 0
    if op.startswith("v_"):
        vop3 = op.endswith("_e64") or op.startswith(("v_mad_", "v_lshl_add", "v_bfe_", "v_mul_lo_", "v_mul_hi_", "v_ashrrev_i64", "v_lshlrev_b64",
                                                     "v_lshrrev_b64", "v_alignbit", "v_add3", "v_xad", "v_lshl_or", "v_and_or", "v_or3", "v_bitop3",
                                                     "v_readlane", "v_writelane", "v_pk_", "v_fma_", "v_perm", "v_add_lshl", "v_lshl_add", "v_cndmask_b32_e64"))
        return (8 if vop3 else 4) + (0 if vop3 else lit)
    return 4 + lit


def _count(ins):
    valu = sum(1 for _, op, _a in ins if op.startswith("v_"))
    nop = sum(1 for _, op, _a in ins if op == "s_nop")
    return {"valu": valu, "s_nop": nop, "other": len(ins) - valu - nop, "slots": len(ins), "code_bytes": sum(_bytes(op, a) for _, op, a in ins)}


def hot_loop_slots(path, kernel="k_msm_comb30"):
    s = open(path).read()
    names = [n for n in re.findall(r"^(_Z\w+):", s, flags=re.M) if kernel in n]
    if not names:
        raise SystemExit("no function matching %r in %s" % (kernel, path))
    name = names[0]
    a = s.index("\n" + name + ":")
    b = s.find(".Lfunc_end", a)
    ins, labels = _instructions(s[a:b if b > 0 else len(s)])
    best = None
    for k, (n, op, args) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = labels.get(args.strip())
            if tgt is not None and tgt < n:
                first = next(i for i, (m, _o, _a) in enumerate(ins) if m > tgt)
                if best is None or k - first > best[1] - best[0]:
                    best = (first, k)
    if best is None:
        raise SystemExit("no backward branch in " + name)
    loop = ins[best[0]:best[1] + 1]
    mads = [i for i, (_n, op, _a) in enumerate(loop) if op.startswith("v_mad_i64_i32")]
    calls = [i for i, (_n, op, _a) in enumerate(loop) if op.startswith("s_swappc")]
    out = {"kernel": name, "hot_loop": _count(loop)}
    if mads:
        # the fast addition is the longest run of multiply-adds no call interrupts
        cuts = [-1] + calls + [len(loop)]
        spans = [[i for i in mads if lo < i < hi] for lo, hi in zip(cuts, cuts[1:])]
        span = max(spans, key=len)
        out["fast_addition_block"] = _count(loop[span[0]:span[-1] + 1])
    return out


def backward_spans(path, kernel="k_msm_comb30"):
    """every backward-branch span of the kernel, outermost last: its counts, multiply-adds, scratch instructions and calls.  A
    kernel that wraps its hot loop in another loop (k_msm_comb30's two passes of a balanced launch) has the wrapping loop as its
    longest span; the hot loop is then read off this list"""
    s = open(path).read()
    names = [n for n in re.findall(r"^(_Z\w+):", s, flags=re.M) if kernel in n]
    if not names:
        raise SystemExit("no function matching %r in %s" % (kernel, path))
    a = s.index("\n" + names[0] + ":")
    b = s.find(".Lfunc_end", a)
    ins, labels = _instructions(s[a:b if b > 0 else len(s)])
    out = []
    for k, (n, op, args) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = labels.get(args.strip())
            if tgt is not None and tgt < n:
                first = next(i for i, (m, _o, _a) in enumerate(ins) if m > tgt)
                loop = ins[first:k + 1]
                row = _count(loop)
                row.update(first=first, last=k, v_mad_i64_i32=sum(1 for _n, o, _a in loop if o.startswith("v_mad_i64_i32")),
                           scratch=sum(1 for _n, o, _a in loop if "scratch" in o), calls=sum(1 for _n, o, _a in loop if o.startswith("s_swappc")))
                out.append(row)
    return sorted(out, key=lambda r: r["slots"])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--spans":
        for r in backward_spans(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "k_msm_comb30"):
            print(json.dumps(r))
    elif len(sys.argv) > 1 and sys.argv[1] == "--slots":
        rest = [x for x in sys.argv[2:] if x != "--json"]
        res = hot_loop_slots(rest[0], rest[1] if len(rest) > 1 else "k_msm_comb30")
        if "--json" in sys.argv:
            print(json.dumps(res, indent=1))
        else:
            print(res["kernel"])
            for k in ("hot_loop", "fast_addition_block"):
                if k in res:
                    print("  %-20s VALU %5d  s_nop %4d  other %4d  slots %5d  code bytes %6d" % ((k,) + tuple(res[k][x] for x in ("valu", "s_nop", "other", "slots", "code_bytes"))))
    else:
        main(sys.argv[1], sys.argv[2:])
