#!/usr/bin/env python3
"""How far behind its load does each `s_waitcnt lgkmcnt(n)` of a kernel sit?  Reads assembly text only; needs no GPU.

On the lone rigid-body wave of k_step a dependent LDS or scalar load costs its whole latency unless enough independent
instructions stand between the load and the wait for it (DESIGN.md section 5 *Bound*).  This tool walks a kernel's text in
order, keeps the queue of outstanding lgkm operations (every `ds_*` and every `s_load*` / `s_buffer_load*`), and for each
`s_waitcnt` with an lgkmcnt(n) field prints the number of instructions since the YOUNGEST operation that wait has to see
finished: the (n + 1)-th youngest outstanding one.  A wait that finds at most n operations outstanding waits for nothing
on the straight-line path and is printed with distance "-".

Assembly: hipcc with the flags of __graft_entry__.build() plus `--cuda-device-only -S` on one unit (method of
profiles/r08_compact_inertia_instructions.txt); a kernel's body is the text from its label to its `.Lfunc_end`.

    python tools/isa_wait_distance.py FILE.s 'k_step<AnymalTraits, true, false, true, 4, true, true>' --loops
    python tools/isa_wait_distance.py FILE.s KERNEL --from .LBB37_12 --to .LBB37_40 [--near 12] [--reads]
    python tools/isa_wait_distance.py FILE.s KERNEL --loop .LBB37_130 [--reads]

KERNEL is the mangled name or the demangled one without its argument list (matched exactly after stripping blanks).
--loops lists the backward branches of the body (label, first and last instruction index, length) so that a loop can be
given to --from / --to by its labels, or, where hipcc has laid blocks of the loop out behind it, to --loop by its header: the
loop is then the set of blocks that hipcc's comments put in it (`in Loop: Header=...`), nested loops included.
--reads lists the LDS reads of the range by address register and offset: the limb table is read through one base
register with offsets (j * LG_JS + J_*) * 4.

The walk is in text order and ignores control flow: a queue carried over a label is that of the fall-through path, and a
loop's first waits see what stood in front of the loop, not what its back edge carries.  Scalar loads may return out of
order, which is why hipcc waits for them with lgkmcnt(0); the distance is counted the same way for both kinds.
"""
import argparse
import re
import subprocess
import sys

LGKM = re.compile(r"^(ds_|s_load_|s_buffer_load_)")
WAIT = re.compile(r"lgkmcnt\((\d+)\)")


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return r.stdout.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
    return list(names)


def squeeze(s):
    s = re.sub(r"^void\s+", "", s.strip())
    s = re.sub(r"\(.*\)$", "", s)                  # argument list of the demangled form
    return re.sub(r"\s+", "", s).replace("(anonymousnamespace)::", "")


def kernel_body(lines, want):
    """(mangled name, [(kind, text)]) with kind 'label' or 'instr', from the kernel's label to its .Lfunc_end."""
    kernels = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    pretty = demangle(kernels)
    hits = [k for k, p in zip(kernels, pretty) if want == k or squeeze(p) == squeeze(want)]
    if len(hits) != 1:
        sys.exit(f"kernel {want!r}: {len(hits)} matches among {len(kernels)} kernels")
    name = hits[0]
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    body = []
    for l in lines[start + 1:]:
        t, _, note = l.partition(";")
        t = t.strip()
        if t.startswith(".Lfunc_end"):
            break
        if re.match(r"^[.\w$]+:$", t):
            body.append(("label", t[:-1], note))
        elif not t:
            m = re.match(r"\s*(%bb\.\d+):(.*)", note)                      # a block entered by falling through
            body.append(("label", m.group(1), m.group(2)) if m else ("note", "", note))
        elif not t.startswith("."):
            body.append(("instr", re.sub(r"\s+", " ", t), ""))
    return name, body


def index_body(body):
    """instructions in order, label -> index of the first instruction behind it, and per instruction its block's label;
    notes: block label -> hipcc's loop annotation of the block (`in Loop: Header=BBn_m`, `Parent Loop BBn_m`, ...)"""
    instrs, labels, block_of, notes, cur = [], {}, [], {}, None
    for kind, t, note in body:
        if kind == "label":
            labels[t] = len(instrs)
            cur = t
            notes[cur] = note
        elif kind == "note":
            if cur is not None and len(instrs) == labels[cur]:
                notes[cur] += " " + note                                     # continuation lines of a loop header's annotation
        else:
            instrs.append(t)
            block_of.append(cur)
    return instrs, labels, block_of, notes


def loop_members(header, notes):
    """labels of the blocks of the loop whose header block is .L<header>: the header, every block annotated `Header=<header>`, and
    the same for every loop nested in it (`Parent Loop <header>`)"""
    header = header.lstrip(".").removeprefix("L")
    heads, grew = {header}, True
    while grew:
        grew = False
        for lab, note in notes.items():
            h = lab.lstrip(".").removeprefix("L")
            if h not in heads and "Loop Header" in note and any(re.search(rf"Parent Loop {re.escape(x)}\b", note) for x in heads):
                heads.add(h); grew = True
    return {lab for lab, note in notes.items()
            if lab.lstrip(".").removeprefix("L") in heads or any(re.search(rf"Header={re.escape(x)}\b", note) for x in heads)}


def loops(instrs, labels):
    out = []
    for i, t in enumerate(instrs):
        m = re.match(r"s_c?branch\w*\s+(\S+)", t)
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            out.append((m.group(1), labels[m.group(1)], i))
    return out


def waits(instrs, lo, hi, inside=None):
    """rows (index, n, distance or None, waited instruction or None) for the waits in [lo, hi) (of the instructions `inside`, if
    given); the queue is walked from 0"""
    queue, rows = [], []
    for i, t in enumerate(instrs[:hi]):
        op = t.split(" ", 1)[0]
        if LGKM.match(op):
            queue.append(i)
        elif op == "s_waitcnt":
            m = WAIT.search(t)
            if not m:
                continue
            n = int(m.group(1))
            show = i >= lo and (inside is None or i in inside)
            if len(queue) > n:
                j = queue[len(queue) - n - 1]
                if show:
                    rows.append((i, n, i - j, instrs[j]))
                queue = queue[len(queue) - n:] if n else []
            elif show:
                rows.append((i, n, None, None))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--from", dest="lo", help="label the range starts at (default: the kernel's label)")
    ap.add_argument("--to", dest="hi", help="label the range ends in front of (default: .Lfunc_end)")
    ap.add_argument("--loop", help="header label of a loop: the range is the loop's blocks as hipcc annotates them, wherever they lie in the text")
    ap.add_argument("--near", type=int, default=12, help="a wait at most this many instructions behind its load counts as near")
    ap.add_argument("--loops", action="store_true", help="list the backward branches of the body and stop")
    ap.add_argument("--reads", action="store_true", help="also list the LDS reads of the range by address register")
    ap.add_argument("--quiet", action="store_true", help="summary lines only")
    a = ap.parse_args()
    with open(a.asm) as f:
        name, body = kernel_body(f.read().splitlines(), a.kernel)
    instrs, labels, block_of, notes = index_body(body)
    print(f"# {a.kernel}  ({name}): {len(instrs)} instructions")
    if a.loops:
        print("# backward branches: label, first .. last instruction, length; [loop header: blocks / instructions of the loop by hipcc's annotation]")
        for lab, s, e in sorted(loops(instrs, labels), key=lambda r: (r[1], -r[2])):
            extra = ""
            if "Loop Header" in notes.get(lab, ""):
                mem = loop_members(lab, notes)
                extra = f"   loop: {len(mem)} blocks, {sum(b in mem for b in block_of)} instructions"
            print(f"{lab:14s} {s:6d} .. {e:6d}  {e - s + 1:6d}{extra}")
        return
    for lab in (a.lo, a.hi, a.loop):
        if lab and lab not in labels:
            sys.exit(f"no label {lab} in this kernel")
    lo, hi, inside = labels[a.lo] if a.lo else 0, labels[a.hi] if a.hi else len(instrs), None
    if a.loop:
        mem = loop_members(a.loop, notes)
        inside = {i for i, b in enumerate(block_of) if b in mem}
    rows = waits(instrs, lo, hi, inside)
    seen = [r for r in rows if r[2] is not None]
    near = [r for r in seen if r[2] <= a.near]
    where = f"loop {a.loop}: {len(inside)} instructions in {len(mem)} blocks" if a.loop else \
        f"range {a.lo or 'kernel label'} .. {a.hi or '.Lfunc_end'}: instructions {lo} .. {hi - 1} ({hi - lo})"
    print(f"# {where}, {len(rows)} lgkmcnt waits, {len(seen)} with a load to wait for, {len(near)} of them at most {a.near} behind it")
    if not a.quiet:
        print("#  index  lgkmcnt  distance  youngest load waited for")
        for i, n, dist, what in rows:
            print(f"{i:8d}  {n:7d}  {'-' if dist is None else dist:>8}  {what or ''}")
    if a.reads:
        by = {}
        for i, t in enumerate(instrs[lo:hi], lo):
            if inside is not None and i not in inside:
                continue
            m = re.match(r"(ds_read\w*)\s+(?:v\d+|v\[\d+:\d+\]|a\d+|a\[\d+:\d+\]),\s*(v\d+)(.*)", t)
            if m:
                by.setdefault(m.group(2), []).append(f"{m.group(1)}{m.group(3)}")
        print("# LDS reads of the range by address register")
        for reg in sorted(by, key=lambda r: -len(by[r])):
            print(f"{reg:5s} {len(by[reg]):4d}  " + "; ".join(by[reg]))


if __name__ == "__main__":
    main()
