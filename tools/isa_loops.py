"""Dev tool: VALU / SALU / DS instructions per iteration of the block kernel's decode loops, from
the gfx950 ISA of dq_inflate3.hip (hipcc -S; the product flags).  A loop is classified by what it
writes: the speculative pass stores a checkpoint word (ds_write_b32), the emit three bytes
(ds_write_b8) and a bitmap bit (ds_or), the re-decode reads the next checkpoint (ds_read_b32) and
the warm-up none of these.  Only loops with two global loads (the two refills of a decode step)
and the common-path (non-SLOW) instantiation are listed.

  python tools/isa_loops.py [extra hipcc flags...]
  python tools/isa_loops.py --resolve [extra hipcc flags...]

--resolve: the resolve's batch loop (the depth-1 loop with the match-start search, v_ffbh, and the
step barriers) split by basic block into the next batch's first hop (up to the first step's byte
reads), the hand-over (four next-pointer reads and no pointer store: the group pointers' adoption),
the jump rounds (blocks that read a next pointer per entry: the scheduler may merge a step's byte
read or store into them), the U store and the rest of the ordered steps.  Counts are per thread
and batch; the rare modulo path (v_rcp_f32) is listed apart.  With -DDQ_RES_SLICE=1 a round is
split up under scalar branches on its live mask: a read block per entry (one ds_read_u16), an
update block per entry (one ds_write_b16) and the blocks of the mask tests between them, which
are all that a round executes when no entry is live; the tool reports the VALU of each kind.
With -DDQ_RES_OCT=1 only the first half of a workgroup's waves takes the first hop, and with
-DDQ_RES_USTORE=1 only the other half stores U lines: blocks behind such a test of the wave's
number are marked "lo waves" / "hi waves", and the last line gives the batch loop's VALU without
the rounds for either half of the waves and their mean (per thread of a workgroup and batch).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.environ.get('DQ_ISA_SRC', os.path.join(ROOT, 'disq_amd', 'csrc', 'dq_inflate3.hip'))


def isa(flags):
    out = os.path.join(tempfile.mkdtemp(), "k.s")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-mllvm",
           "-amdgpu-sched-strategy=max-ilp", "--cuda-device-only", "-S", "-o", out, SRC] + flags
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel(text, prefix):
    lines = text.split("\n")
    a = next(i for i, l in enumerate(lines) if l.startswith(prefix))
    b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[a:b]


def loops(lines):
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):.*Depth=(\d+)", l)
        if not m:
            continue
        name = m.group(1)
        last = None
        for j in range(i + 1, min(len(lines), i + 3000)):
            if re.search(r"s_(cbranch_\w+|branch)\s+" + re.escape(name) + r"$", lines[j].strip()):
                last = j
        if last is None:
            continue
        body = [x.strip() for x in lines[i + 1:last + 1]
                if x.strip() and not x.strip().startswith((";", "."))]
        yield name, body


def classify(body):
    has = lambda op: any(x.startswith(op) for x in body)  # noqa: E731
    if has("ds_write_b8") and has("ds_or"):
        return "emit"
    if has("ds_write_b32"):
        return "spec"
    if has("ds_read_b32"):
        return "redo"
    return "warm-up"


def resolve(ker):
    best = None
    for name, body in loops(ker):
        if (any(x.startswith("v_ffbh") for x in body) and any(x.startswith("ds_read_u16") for x in body)
                and sum(x.startswith("s_barrier") for x in body) >= 2):
            if best is None or len(body) > len(best[1]):
                best = (name, body)
    a = next(i for i, l in enumerate(ker) if l.startswith(best[0] + ":"))
    # -DDQ_RES_OCT=1: code that only the first waves of a workgroup run (the first hop: a scalar
    # compare of the wave's number, v_readfirstlane, and a branch over it) or only the others (the
    # U stores of -DDQ_RES_USTORE=1: the same compare folded into the exec mask) is split off
    # into blocks of its own, marked "lo" and "hi"
    blocks, cur = [], None
    n = 0
    text = [l.strip() for l in ker[a:]]
    text = [x for x in text if x and (re.match(r"^\.LBB\d+_\d+:", x) or not x.startswith((";", ".")))]
    gate, gate_end = None, None
    for i, x in enumerate(text):
        m = re.match(r"^(\.LBB\d+_\d+):", x)
        if m:
            if m.group(1) == gate_end:
                gate, gate_end = None, None
            cur = [m.group(1), [], gate]
            blocks.append(cur)
            continue
        cur[1].append(x)
        n += 1
        if n >= len(best[1]):
            break
        if gate is None and re.match(r"s_cbranch_(scc1|execz)\s", x):
            back = text[max(0, i - 8):i]
            k = [j for j, y in enumerate(back) if re.match(r"s_cmp_gt_i32 s\d+, \d+$", y)]
            if k and any(y.startswith("v_readfirstlane_b32") for y in text[max(0, i - 12):i]):
                direct = back[k[-1] + 1:] == []  # the branch tests the compare itself: skips the upper waves
                if direct or x.startswith("s_cbranch_execz"):
                    gate, gate_end = ("lo" if direct else "hi"), x.split()[-1]
                    cur = [cur[0] + "'", [], gate]
                    blocks.append(cur)
    cnt = lambda b, op: sum(x.startswith(op) for x in b)  # noqa: E731
    state, tot, rounds = "first hop", {}, []
    split = {"read": [], "update": [], "test": []}
    print(f"resolve batch loop {best[0]}: {len(best[1])} instructions")
    waves = {None: {}, "lo": {}, "hi": {}}  # kind -> VALU, by the waves that run the block
    for name, b, gate in blocks:
        if not b:
            continue
        if state == "first hop" and cnt(b, "ds_read_u8"):
            state = "steps"
        kind = state
        if cnt(b, "v_rcp_f32"):
            kind = "modulo path"
        elif state == "steps" and cnt(b, "ds_read_u16") >= 4 and not cnt(b, "ds_write_b16"):
            kind = "hand-over"
        elif state == "steps" and cnt(b, "ds_read_u16") >= 4:
            kind = "jump round"
            rounds.append(cnt(b, "v_"))
        elif state == "steps" and cnt(b, "ds_read_u16") == 1 and cnt(b, "ds_") == 1:
            kind = "round read"
            split["read"].append(cnt(b, "v_"))
        elif state == "steps" and cnt(b, "ds_write_b16") == 1 and not cnt(b, "ds_read"):
            kind = "round update"
            split["update"].append(cnt(b, "v_"))
        elif state == "steps" and cnt(b, "s_bitcmp1_b32") and not cnt(b, "ds_") and not cnt(b, "s_barrier"):
            kind = "round test"
            split["test"].append(cnt(b, "v_"))
        elif cnt(b, "global_store") and (state == "steps" or gate == "hi"):
            kind = "U store"
        v, sa, d = cnt(b, "v_"), cnt(b, "s_"), cnt(b, "ds_")
        t = tot.setdefault(kind, [0, 0, 0, 0])
        for i, q in enumerate((v, sa, d, cnt(b, "v_ffbh"))):
            t[i] += q
        waves[gate][kind] = waves[gate].get(kind, 0) + v
        if v + d > 3 or kind.startswith("round "):
            print(f"  {name:12s} {kind:12s} VALU {v:4d}  SALU {sa:4d}  DS {d:3d}  ffbh {cnt(b, 'v_ffbh')}"
                  f"  ds_write_b64 {cnt(b, 'ds_write_b64')}  barriers {cnt(b, 's_barrier')}"
                  + (f"  {gate} waves" if gate else ""))
    for k, t in tot.items():
        print(f"{k:12s} VALU {t[0]:4d}  SALU {t[1]:4d}  DS {t[2]:3d}  ffbh {t[3]}")
    if rounds:
        print("jump rounds:", " ".join(map(str, rounds)), "VALU each")
    # per thread and batch without the rounds (a wave runs as many as its chains need; the blocks
    # above are their unrolled copies) and the modulo path: the lower and the upper half of the
    # workgroup's waves, and their mean (the workgroup's sum per batch is that times its waves)
    fixed = [k for k in tot if k not in ("jump round", "modulo path") and not k.startswith("round ")]
    lo = sum(waves[None].get(k, 0) + waves["lo"].get(k, 0) for k in fixed)
    hi = sum(waves[None].get(k, 0) + waves["hi"].get(k, 0) for k in fixed)
    print(f"batch loop without rounds, VALU per thread and batch: lower waves {lo}, upper waves {hi}, "
          f"mean {(lo + hi) / 2:.1f} ({', '.join(fixed)})")
    if split["read"] or split["update"]:
        r, u = max(split["read"] or [0]), max(split["update"] or [0])
        print(f"split rounds: {len(split['read'])} read blocks of at most {r} VALU (a read block holds the next "
              f"entry's mask test too), {len(split['update'])} update blocks of at most {u} VALU:")
        print(f"  a live entry costs at most {r + u} VALU; a round with no live entry runs the mask tests alone: "
              f"{max(split['read'] + split['test'] + [0])} VALU in any block of them")


def main():
    if "--resolve" in sys.argv[1:]:
        text = isa([a for a in sys.argv[1:] if a != "--resolve"])
        return resolve(kernel(text, "_ZN2dq12_GLOBAL__N_120inflate_block_kernelILb0"))
    text = isa(sys.argv[1:])
    ker = kernel(text, "_ZN2dq12_GLOBAL__N_120inflate_block_kernelILb0")
    seen = {}
    for name, body in loops(ker):
        g = sum(x.startswith("global_load") for x in body)
        if g != 2 or any(x.startswith("v_bfrev_b32") for x in body):
            continue  # not a decode step, or the canonical (SLOW) instantiation
        v = sum(x.startswith("v_") for x in body)
        s = sum(x.startswith("s_") for x in body)
        d = sum(x.startswith("ds_") for x in body)
        kind = classify(body)
        if kind not in seen or v < seen[kind][1]:
            seen[kind] = (name, v, s, d)
    for k in ("warm-up", "spec", "redo", "emit"):
        if k in seen:
            name, v, s, d = seen[k]
            print(f"{k:8s} {name:12s} VALU {v:4d}  SALU {s:4d}  DS {d:3d}")


if __name__ == "__main__":
    main()
