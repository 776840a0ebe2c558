"""Split planning at its edges: the split's block range by search (plan_blocks_kernel,
dqc::last_block_le) and the first record of a split found by a head launch and the interleaved
workgroups (first_record_kernel), against the oracle's partitions.

The small file is a few hundred BGZF members of a few hundred bytes with a run of empty members
and one 40 KB stored member; the split sizes put a split end exactly on a member start, one byte
before and one after it, at the first, inside and behind a run of empty members, and several whole
splits inside the stored member (splits without a member start).  The last split of every size
ends behind the last member.  The long-read file (2,000 records, reads of up to 2 Mb) is read with
a split size whose second split starts inside a read, further from its first record than the
head launch looks."""
import bisect
import functools

import numpy as np
import pytest

from disq_amd import _lib, synth
from oracle import oracle as O

import bamutil as B
import baiutil
import reccases as R

HDR = R.header([("chr1", 100_000_000)])
N_RUN = 6          # empty members per run
BIG = 40000        # payload of the stored member


@functools.lru_cache(maxsize=None)
def members_file():
    """(bam, member start positions, (first, past-the-end) position of the run of empty members,
    the stored member's position)."""
    lay = R.layout(HDR, [R.filler(44 + (37 * i) % 400, pos=100 * i) for i in range(700)])
    u = lay.stream
    out, at, marks, i = [], 0, {}, 0
    while at < len(u):
        n = BIG if i == 120 else 300 + (53 * i) % 400
        if i == 120:
            marks["big"] = sum(map(len, out))
        out.append(B.bgzf_member(u[at:at + n], 0 if i == 120 else 6))
        at += n
        i += 1
        if i == 40:
            a = sum(map(len, out))
            out.append(B.EOF_BLOCK * N_RUN)
            marks["run"] = (a, a + 28 * N_RUN)
    bam = b"".join(out) + B.EOF_BLOCK
    pos, _, _ = baiutil._blocks(bam)
    return bam, pos, marks["run"], marks["big"]


def split_sizes():
    bam, pos, (r0, r1), big = members_file()
    p = pos[25]  # a member start a few KB into the file: about twenty splits of that size
    return {"ends_on_member": p, "ends_before_member": p - 1, "ends_after_member": p + 1,
            "ends_on_run": r0, "ends_inside_run": r0 + 28 * 3 + 1, "ends_behind_run": r1,
            "ends_on_run_last": r1 - 28}


def test_members_file_reaches_the_edges():
    bam, pos, run, big = members_file()
    assert 200 < len(pos) < 800 and len(bam) < 1 << 20
    assert B.inflate_all(bam) == R.layout(HDR, [R.filler(44 + (37 * i) % 400, pos=100 * i) for i in range(700)]).stream
    assert all(x in pos for x in range(run[0], run[1], 28)) and run[1] in pos
    sizes = split_sizes()
    assert len(set(sizes.values())) == len(sizes)
    p = sizes["ends_on_member"]
    assert p in pos and p - 1 not in pos and p + 1 not in pos
    nxt = pos[pos.index(big) + 1]
    for name, s in sizes.items():
        splits = O.path_splits(len(bam), s)
        assert splits[0][1] == s and splits[-1][1] >= pos[-1]  # the last split ends behind the last member
        # whole splits inside the stored member: no member start in them
        empty = [(a, b) for a, b in splits if bisect.bisect_left(pos, a) == bisect.bisect_left(pos, b)]
        assert any(big < a and b < nxt for a, b in empty), name
    assert sizes["ends_on_run"] == run[0] and sizes["ends_behind_run"] == run[1]


def digests_vs_oracle(data, split):
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.open_bytes(data)
        st = c.run_resident()
        cnt, dig = c.partition_digests()
    splits = O.path_splits(len(data), split)
    ocnt, odig, _ = O.run_partitions(data, splits, 8)
    assert len(cnt) == len(splits)
    assert np.array_equal(cnt, ocnt), split
    assert np.array_equal(dig, odig), split
    return st, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(split_sizes()))
def test_gpu_member_edges(name):
    bam = members_file()[0]
    st, cnt = digests_vs_oracle(bam, split_sizes()[name])
    # (a record at the start of a member that a split ends on belongs to both partitions, as in
    # the reference: blocks while start <= split end)
    assert 700 <= int(cnt.sum()) <= 701


def head_positions():
    """first_record_kernel's head launch, from the source."""
    src = open(R.CSRC + "/dq_kernels.hip").read()
    return int(R._find(src, r"#define DQ_FR_HEAD (\d+)", "DQ_FR_HEAD").group(1))


@pytest.mark.gpu
def test_gpu_long_read_split_starts_inside_a_read():
    s = synth.generate(2000, seed=41, shape=synth.LONGREAD, records_per_chunk=250, nthreads=8)
    assert s.n_records == 2000
    split = 8 << 20
    ob = O.OracleBam(s.bam)
    # the second split's first record lies further into its first block's bytes than the head
    # launch looks and than one interleaved round of the sixteen workgroups: it starts inside a read
    (s1, e1, chunk) = ob.plan(split)[1]
    blocks = ob.split_blocks(s1, e1)
    assert chunk is not None and blocks
    vstart = int(chunk[0])
    first = blocks[0][0]
    upto = 0
    for p, _, us in blocks:
        if p == vstart >> 16:
            break
        upto += us
    assert p == vstart >> 16 and first >= s1
    dist = upto + (vstart & 0xffff)
    assert dist > max(head_positions(), 16 * 256), dist
    st, cnt = digests_vs_oracle(s.bam, split)
    assert int(cnt.sum()) == 2000 and len(cnt) > 4
