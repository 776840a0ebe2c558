"""The BGZF block chain by windows on the GPU (chain_walk / chain_link / chain_fix kernels,
dq_chain_core.h) and the planners over listed candidate ranges (split_cands): fixtures whose
members lie where the windowed walk can go wrong (tests/chaincases.py), read through the text path
(any bytes are lines there) and the BAM path, against the oracle and against the Python
restatement of the serial walk.

Every check runs under the product library in this process (windows sized per file: 4 KiB for
these files, so every multiple of 4096 is a window edge) and, through this file run as a script in
a child process, under the two variant builds of `make chainw`: windows of 64 KiB whatever the
size, as a large file is walked (a 300 KB file has five of them, each with a block start, and the
dense file takes the give-up and the retry with fine windows), and the same with the planners'
candidate ranges cut to one chunk so that planning takes its full-scan retry.

What the product library does not walk here is a wide window: every fixture, the 3 x 1 MiB + 1
one included, is under 64 MB and so gets 4 KiB windows; the sizes and edges "at 1 MiB" are edges
of 4 KiB windows too, not of a 1 MiB walk.  Wide windows run at 64 KiB under the variants (the
kernels are the same code for every W) and at 1 MiB only in the benchmark, whose digest is the
check there.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from disq_amd import _lib, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

import bamutil as B  # noqa: E402
import chaincases as K  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
WINDOWS = (K.W_SMALL, 1 << 20)  # the variant builds' window and the product's widest
ONE_SPLIT = 1 << 30


# ---------------------------------------------------------------- helpers
def gpu_text(data, split):
    """(n_blocks, [[(value offset, value length)] per partition])."""
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.text_open_bytes(data)
        st = c.text_run(True)
        b = c.text_read(True)
    po = b["part_offset"].tolist()
    rows = list(zip(b["line_offset"].tolist(), b["line_len"].tolist()))
    return st.n_blocks, [rows[a:z] for a, z in zip(po, po[1:])]


def text_vs_oracle(data, split):
    ot = O.OracleText(data)
    want = [list(zip(vs.tolist(), vl.tolist())) for vs, vl in ot.read_partitions(split, True)]
    nblk, got = gpu_text(data, split)
    assert nblk == len(K.chain_serial(data))
    assert got == want


def text_vs_restatement(data):
    """One split over a file that may end badly: the lines of the serial chain's blocks."""
    chain = K.chain_serial(data)
    u = b"".join(zlib.decompress(data[p + 18:p + c - 8], -15) for p, c, _ in chain)
    assert [len(zlib.decompress(data[p + 18:p + c - 8], -15)) for p, c, _ in chain] == [x[2] for x in chain]
    want, at = [], 0
    for line in K.lines_of(u):
        want.append((at, len(line)))
        at += len(line) + 1
    nblk, got = gpu_text(data, ONE_SPLIT)
    assert nblk == len(chain)
    assert got == [want]


def bam_vs_oracle(data, split, voff_shift=0, ref=None):
    ob = O.OracleBam(ref if ref is not None else data)
    parts = [p for p in ob.read_partitions(split)] if ref is None else [ob.read_all()]
    want = np.concatenate(parts)
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.open_bytes(data)
        b = c.read(with_raw=False)
        nblk = c.stats().n_blocks
    assert nblk == len(K.chain_serial(data))
    assert np.array_equal(b["voffset"], want["voffset"] + np.uint64(voff_shift << 16))
    assert np.array_equal(b["hash"], want["hash"])
    if ref is None:
        assert np.diff(b["part_offset"]).tolist() == [len(p) for p in parts]


# ---------------------------------------------------------------- the checks
def check_sizes_and_edges():
    for W in WINDOWS:
        for total in (W - 1, W, W + 1, 3 * W + 1):  # one under, exactly, one over; three windows and a byte
            data, _ = K.sized_text_file(total)
            text_vs_oracle(data, 100000)
        for boundary in (W - 1, W, W + 1):          # a member starts one before, at, one after a window start
            data, _ = K.edge_text_file(boundary, nwin=2 if W > K.W_SMALL else 4)
            text_vs_oracle(data, 70001)
        # a member of the full 65536 bytes over a window start: no block starts in the window's
        # first 65000 bytes
        data, _ = K.edge_text_file(W - 500, nwin=2, rest=65505)
        starts = [b[0] for b in K.chain_serial(data)]
        assert W - 500 in starts and not any(W <= s < W + 65000 for s in starts)
        text_vs_oracle(data, 140000)
    text_vs_oracle(K.stored_member(K.text_stream(500)) + K.EOF_BLOCK, ONE_SPLIT)  # a single member
    nblk, got = gpu_text(K.EOF_BLOCK, ONE_SPLIT)                               # only the EOF block
    assert nblk == 1 and got == [[]]


def check_fakes_at_window_starts():
    """A complete member in stored payload exactly at a window's first byte: that window speculates
    it, its link breaks, the repair gives the serial chain; the planner of a split that starts just
    before an empty one answers as the reference does (the text reader fails on it)."""
    data_fake = K.deflated_member(b"hello, world")
    for fakes, wins in (([K.EOF_BLOCK], (2,)), ([data_fake], (2,)), ([K.EOF_BLOCK, K.EOF_BLOCK], (2, 3))):
        data, stream = K.fake_at_window_text(fakes, wins)
        text_vs_oracle(data, 100000)   # no split starts at a fake
        text_vs_oracle(data, ONE_SPLIT)
    data, _ = K.fake_at_window_text([K.EOF_BLOCK], (2,))
    split = 2 * K.W_SMALL - 7          # split 1 starts 7 bytes before the fake member
    with pytest.raises(O.OracleError):
        O.OracleText(data).read_partitions(split, True)
    with pytest.raises(_lib.DqError, match="not on the block chain"):
        gpu_text(data, split)
    # the BAM planner hops over an empty fake member at a split start (tests/test_adversarial.py)
    from test_adversarial import fake_header_bam
    bam, fake, _ = fake_header_bam("eof")
    bam_vs_oracle(bam, fake - 7)
    bam, fake, _ = fake_header_bam("broken")
    bam_vs_oracle(bam, fake - 7)


def check_dense_members():
    """Results only; the times are in profiles/r11j_small_files.txt (the first file: scan stage
    0.246 ms against the parent's 0.268 ms, the pipeline level with the parent's at 3.80 ms).  Under the 64 KiB variants the first file makes the count
    pass give up and the chain is walked again with 4 KiB windows."""
    one = open(os.path.join(GOLDEN, "1.bam"), "rb").read()
    n = 20000  # 560,000 bytes of empty members in front of the data: 20,000 hops for one window's walk
    bam_vs_oracle(K.EOF_BLOCK * n + one, ONE_SPLIT, voff_shift=28 * n, ref=one)
    r = synth.generate(300, seed=5, nthreads=2)
    small = B.bgzf(B.inflate_all(r.bam), 6, block_u=100)  # members of about 100 bytes
    assert len(K.chain_serial(small)) > 500
    bam_vs_oracle(small, 30000)


def check_chains_that_end_early():
    good = [K.stored_member(K.text_stream(20000, s)) for s in range(8)]  # 160 KB: three small windows
    # XLEN != 6 with a second subfield: the guesser takes the member, htsjdk does not
    odd = K.stored_member(b"odd\n", extra=b"XY\x02\x00\x07\x07")
    text_vs_restatement(b"".join(good[:5]) + odd + b"".join(good[5:]) + K.EOF_BLOCK)
    whole = b"".join(good)
    last = len(whole) - len(good[-1])
    for cut in list(range(last + 1, last + 19)) + list(range(len(whole) - 8, len(whole))):
        text_vs_restatement(whole[:cut])                      # the last member cut in its header, its trailer
    text_vs_restatement(whole + K.EOF_BLOCK + b"garbage" * 9)  # trailing garbage
    text_vs_restatement(whole)                                # no EOF block


def check_shards_and_spans():
    from test_parallel import _check_shards_oracle
    from test_span import gpu_span, oracle_parts
    one = open(os.path.join(GOLDEN, "1.bam"), "rb").read()
    # shards whose bytes begin and end inside members, already in device memory
    _check_shards_oracle(one, 65536, 3, 1 << 20, device_bytes=True)
    a = synth.generate(20000, shape=synth.ANYSAM, bai=True)
    assert len(a.bam) > 2 * K.W_SMALL
    ob = O.OracleBam(a.bam)
    for ivs in ([(20, 5000, 9999), (20, 20000, 22999)], [(20, 300000, 300500), (3, 1, 100)]):
        st, cnt, dig = gpu_span(a.bam, a.bai, 40000, ivs)
        ocnt, odig = oracle_parts(ob, 40000, ivs, a.bai)
        assert np.array_equal(cnt, ocnt) and np.array_equal(dig, odig), ivs


def shard_read(data, base, length, p0, p1, split, header):
    """The shard's bytes in device memory through open_shard_device: (records, blocks)."""
    import torch
    d = data[base:base + length]
    t = torch.zeros(len(d) + 4096, dtype=torch.uint8, device="cuda:0")
    t[:len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.open_shard_device(t.data_ptr(), len(d), base, len(data), p0, p1, header)
        b = c.read(with_raw=False)
        return len(b["voffset"]), c.stats().n_blocks


def check_shard_chain_starts():
    """A shard's chain starts at the first position from byte 0 that the guesser returns.  The
    expected errors are the parent commit's on the same bytes (profiles/r11f_shard_probe.txt)."""
    one = open(os.path.join(GOLDEN, "1.bam"), "rb").read()
    with _lib.Context() as hc:
        h1 = hc.header_from_prefix(one[:1 << 20])
    starts = [b[0] for b in K.chain_serial(one)]
    split = 65536
    # no hit at all: 2000 bytes inside one member; the chain start is L and the chain is empty
    p0 = next(p for p in range(1, 6) if not any(p * split <= x < p * split + 2000 for x in starts))
    assert K.first_guess(one[p0 * split:p0 * split + 2000]) == 2000
    with pytest.raises(_lib.DqError, match="no BGZF blocks found"):
        shard_read(one, p0 * split, 2000, p0, p0 + 1, split, h1)
    # the halo ends inside the member that spans the last split end: no block after the split
    with pytest.raises(_lib.DqError, match="shard halo too small: no BGZF block after the last split"):
        shard_read(one, 0, 66000, 0, 1, split, h1)
    # a fake (empty) member in stored payload is the shard's first hit: the chain starts on it and
    # window 0's walk stops behind it
    from test_adversarial import fake_header_bam
    bam, fake, _ = fake_header_bam("eof")
    with _lib.Context() as hc:
        h2 = hc.header_from_prefix(bam[:1 << 20])
    sp = fake - 7
    assert K.first_guess(bam[sp:]) == 7 and len(K.chain_serial(bam[sp:], 7)) == 1
    assert shard_read(bam, sp, len(bam) - sp, 1, 2, sp, h2) == (0, 1)  # no records, the fake block alone


CHECKS = [check_sizes_and_edges, check_fakes_at_window_starts, check_dense_members,
          check_chains_that_end_early, check_shards_and_spans, check_shard_chain_starts]


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_product_windows(check):
    check()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["chainw", "chainfull"])
def test_variant_builds(variant):
    """The same checks under 64 KiB windows; chainfull must have taken the planners' full-scan retry
    (the full scan reports itself under DQ_DEBUG), chainw must never have."""
    lib = os.path.join(ROOT, "disq_amd", "_build", f"libdisq_gpu_{variant}.so")
    if not os.path.exists(lib):
        pytest.fail(f"libdisq_gpu_{variant}.so is not built (make -C disq_amd/csrc chainw)")
    env = dict(os.environ, DQ_GPU_LIB=lib, DQ_DEBUG="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:] + err[-3000:]
    assert ("[dq] scan " in err) == (variant == "chainfull")
    assert "[dq] chain dense 65536" in err  # the dense file gave up its wide windows


if __name__ == "__main__":
    for f in CHECKS:
        f()
        print("ok", f.__name__, flush=True)
