"""ONE path through the entry loop of a kernel of the built library, block by block: vector instructions, v_mov and s_nop per
block and in all.  tools/kloop.py counts the whole loop, rare sides included (guard re-test, exact tier, exponential tier); this
follows the handful of branch decisions that define a path -- e.g. the ordinary one: Taylor-tier row, no guard trip, no exact-tier
entry -- from the block that holds the entry's Gaussian around the loop and back to it.

    python tools/kpath.py <kernel substring> --path tnnt...   [--anchor OPCODE] [--nth K] [--lib path] [--dump]
    python tools/kpath.py <kernel substring> --enumerate      [--nth K] [--max-vector N] [--limit N]

The walk starts at the basic block with the K-th occurrence of the anchor opcode (default v_exp_f32; count through the kernel's
exponentials until the block is the entry's Gaussian -- its four v_exp_f32 sit together; the backward holds its entry loop twice,
the pass on the walk summary first) and works on the kernel's whole control-flow graph: the compiler rotates loops, gives them
several latches and moves their rare blocks far away, so an address range does not hold a loop.  --path has one letter per
CONDITIONAL branch met on the way, in order: t = taken, n = not taken; unconditional branches are followed, calls stepped over.
The walk ends where it meets a block it has been through -- the cycle from there on is what is counted --, where the kernel ends,
or when the letters run out (the next branch is then printed, so a path can be written down one decision at a time).
--enumerate lists every cycle-free way from the anchor's block back to it (walks are given up beyond --max-vector vector
instructions) with its letters and totals, fewest vector instructions last: the ordinary path is the one with no call that leaves
the rare blocks out.  Opcodes are only counted by class (v_*, v_mov*, s_nop, calls, memory instructions: the
backward's ordinary path is the one that passes both of an entry's atomics)."""
import os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "lib.so")
        with open(lib, "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", dst], cwd=tmp, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f], cwd=tmp,
                                 capture_output=True, text=True).stdout
            for blk in re.split(r"\n(?=[0-9a-f]+ <)", dis):
                m = re.match(r"[0-9a-f]+ <(\S+)>:", blk)
                if m:
                    yield m.group(1), blk


def branch_target(a, t):
    b = re.match(r"s_c?branch\S*\s+(\d+)", t)
    if not b:
        return None
    off = int(b.group(1)); off = off - 65536 if off >= 32768 else off
    return a + 4 + 4 * off


class Loop:
    """the kernel's basic blocks; `start`: the block that holds the K-th occurrence of the anchor opcode"""
    def __init__(self, blk, anchor, nth):
        self.ins = [(int(a, 16), t.strip()) for t, a in re.findall(r"^\s+(\S.*?)\s*// ([0-9A-Fa-f]+):", blk, flags=re.M)]
        anchors = [a for a, t in self.ins if t.split()[0].startswith(anchor)]
        if not anchors:
            raise SystemExit(f"no {anchor}")
        first = anchors[min(nth, len(anchors) - 1)]
        body = self.ins
        self.lo, self.hi = body[0][0], body[-1][0]
        leaders = {self.lo}
        for i, (a, t) in enumerate(body):
            tgt = branch_target(a, t)
            if tgt is not None:
                if self.lo <= tgt <= self.hi:
                    leaders.add(tgt)
                if i + 1 < len(body):
                    leaders.add(body[i + 1][0])
            elif t.startswith(("s_endpgm", "s_setpc")) and i + 1 < len(body):
                leaders.add(body[i + 1][0])
        self.blocks, cur = {}, None
        for a, t in body:
            if a in leaders:
                cur = a; self.blocks[cur] = []
            self.blocks[cur].append((a, t))
        self.order = sorted(self.blocks)
        self.start = max(b for b in self.order if b <= first)

    def next_of(self, b):
        i = self.order.index(b)
        return self.order[i + 1] if i + 1 < len(self.order) else None  # (None: falls out of the loop)

    def step(self, b, decide):
        """-> (next block or None = left the loop, letter consumed or '')"""
        a, t = self.blocks[b][-1]
        tgt = branch_target(a, t)
        if t.startswith(("s_endpgm", "s_setpc")):
            return None, ""
        if tgt is None:
            return self.next_of(b), ""
        if t.startswith("s_branch"):
            return (tgt if self.lo <= tgt <= self.hi else None), ""
        d = decide(a, t)
        if d is None:
            return "stop", ""
        nxt = tgt if d == "t" else self.next_of(b)
        return (nxt if nxt is not None and self.lo <= nxt <= self.hi else None), d


def count(block):
    ops = [t.split()[0] for a, t in block]
    return dict(n=len(ops), v=sum(o.startswith("v_") for o in ops), mov=sum(o.startswith("v_mov") for o in ops),
                nop=sum(o == "s_nop" for o in ops), call=sum(o.startswith("s_swappc") for o in ops),
                mem=sum(o.startswith(("global_", "flat_", "buffer_", "scratch_")) for o in ops))


def total(L, blocks):
    tot = dict(n=0, v=0, mov=0, nop=0, call=0, mem=0)
    for b in blocks:
        for k, v in count(L.blocks[b]).items():
            tot[k] += v
    return tot


def enumerate_paths(L, limit, max_vector):
    """every cycle-free way from the anchor's block back to it, as (letters, blocks); a walk is given up beyond max_vector"""
    found = []

    def go(b, seen, letters, v):
        if len(found) >= limit or v > max_vector:
            return
        for d in "tn":
            used = []
            nxt, got = L.step(b, lambda a, t: used.append(d) or d)
            if nxt == L.start:
                found.append((letters + got, seen + [b]))
            elif nxt is not None and nxt not in seen and nxt != b:
                go(nxt, seen + [b], letters + got, v + count(L.blocks[nxt])["v"])
            if not used:
                break  # (no conditional branch at the end of this block: one successor)

    go(L.start, [], "", count(L.blocks[L.start])["v"])
    return found


def main():
    argv = sys.argv[1:]
    def opt(name, default=None):
        if name in argv:
            i = argv.index(name); v = argv[i + 1]; del argv[i:i + 2]; return v
        return default
    def flag(name):
        if name in argv:
            argv.remove(name); return True
        return False
    anchor, nth = opt("--anchor", "v_exp_f32"), int(opt("--nth", "0"))
    lib = opt("--lib") or os.environ.get("GSGEN_HIP_LIB") or os.path.join(os.path.dirname(__file__), "..", "gsgen_amd", "lib", "libgsgen_hip.so")
    path, limit, max_vector = opt("--path"), int(opt("--limit", "4000")), int(opt("--max-vector", "400"))
    enum, dump = flag("--enumerate"), flag("--dump")
    sub = argv[0]
    for name, blk in kernels(lib):
        if sub in name and name.startswith("_ZN2gs"):
            break
    else:
        raise SystemExit("no such kernel")
    L = Loop(blk, anchor, nth)
    print(name)
    print(f"{len(L.blocks)} blocks; occurrence {nth} of {anchor} is in block {hex(L.start)}")
    if enum:
        rows = []
        for letters, blocks in enumerate_paths(L, limit, max_vector):
            rows.append((total(L, blocks), letters, len(blocks)))
        rows.sort(key=lambda r: -r[0]["v"])
        for tot, letters, nb in rows:
            print(f"  vector {tot['v']:4d}  v_mov {tot['mov']:3d}  s_nop {tot['nop']:3d}  calls {tot['call']}  memory {tot['mem']}  blocks {nb:3d}  --path {letters or '-'}")
        return
    letters = list((path or "").replace("-", ""))
    b, walked, used = L.start, [], ""
    while True:
        walked.append(b)
        def decide(a, t):
            if not letters:
                print(f"  (letters used up at {hex(a)} {t})")
                return None
            return letters.pop(0)
        nxt, got = L.step(b, decide)
        used += got
        if nxt == "stop":
            end = "stopped"; break
        if nxt is None:
            end = "left the kernel"; break
        if nxt in walked:
            end = "back at " + hex(nxt); walked = walked[walked.index(nxt):]; break  # (what is counted: the cycle)
        b = nxt
    for b in walked:
        c = count(L.blocks[b])
        print(f"  block {hex(b)}: {c['n']:3d} instructions, vector {c['v']:3d}, v_mov {c['mov']:2d}, s_nop {c['nop']:2d}" + (f", calls {c['call']}" if c["call"] else "") + (f", memory {c['mem']}" if c["mem"] else "")
              + f"   ends: {L.blocks[b][-1][1]}")
        if dump:
            for a, t in L.blocks[b]:
                print("     ", hex(a), t)
    tot = total(L, walked)
    print(f"path {used or '-'} ({end}): {len(walked)} blocks, {tot['n']} instructions, vector {tot['v']}, v_mov {tot['mov']}, s_nop {tot['nop']}, calls {tot['call']}, memory {tot['mem']}")


main()
