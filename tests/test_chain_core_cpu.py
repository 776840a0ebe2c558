"""The chain core (disq_amd/csrc/dq_chain_core.h) on the CPU through tools/chain_check.cpp: the
windowed walk with its link rule and repair, and the planners' guess loop over a candidate list
that covers byte ranges only, against the Python restatement of the serial walk and of
guessNextBGZFPos (tests/chaincases.py).  The restatement is held against the oracle on the golden
files first.  The tool runs with small windows (any W), so every link case costs a few KB.

What this covers is the shared core: htsjdk_block, guesser_at, walk_window (which the repair
kernel calls), the link rule and cand_next, in the orchestration the kernels follow.  The count and
emit kernel's own walk -- the same steps with the headers read from an LDS-staged piece where
members are short -- is kernel code outside the core: it is held against the same restatement by
tests/test_bgzf_chain.py on the GPU (dense members, and under the bounds-checked library)."""
import os
import subprocess

import pytest

from oracle import oracle as O

import chaincases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disq_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", "-Wall", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "chain_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    """Built with the sanitizers and run directly: every case below is also a sanitizer run."""
    return _build(tmp_path_factory.mktemp("chaincore"), "chain_check_san",
                  ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run_chain(tool, path, W, start=0):
    out = subprocess.run([tool, "chain", str(path), str(W), str(start)], check=True,
                         stdout=subprocess.PIPE).stdout.decode().split("\n")
    n, broken = map(int, out[0].split())
    return [tuple(map(int, l.split())) for l in out[1:1 + n]], broken


def run_guess(tool, path, p, e, ranges=()):
    out = subprocess.run([tool, "guess", str(path), str(p), str(e), *[str(x) for r in ranges for x in r]],
                         check=True, stdout=subprocess.PIPE).stdout.decode().strip()
    return out if out in ("null", "unknown") else tuple(map(int, out.split()))


GOLDEN_BGZF = sorted(f for f in os.listdir(GOLDEN) if f.endswith((".bam", ".bgz")))


# ---------------------------------------------------------------- the restatement vs the oracle
@pytest.mark.parametrize("name", GOLDEN_BGZF)
def test_restatement_against_oracle(name):
    d = open(os.path.join(GOLDEN, name), "rb").read()
    ob = O.OracleBam(d)
    # BgzfBlockSource's blocks of a split covering the file are the chain of a well-formed file
    assert K.chain_serial(d) == ob.split_blocks(0, len(d))
    step = max(1, len(d) // 97)
    for p in list(range(0, len(d), step)) + [len(d) - 28, len(d) - 27, len(d) - 3]:
        for end in (p + 1, p + 5000, len(d), 1 << 40):
            g = K.guess_next(d, p, end)
            assert g == ob.guess_next_bgzf(p, end), (p, end)


# ---------------------------------------------------------------- the windowed walk
def _check_all_windows(tool, tmp_path, d, windows, start=0, want_broken=None):
    f = tmp_path / "f.bin"
    f.write_bytes(d)
    want = K.chain_serial(d, start)
    for W in windows:
        got, broken = run_chain(tool, f, W, start)
        assert got == want, W
        if want_broken is not None:
            assert broken == want_broken, W
    return want


@pytest.mark.parametrize("name", GOLDEN_BGZF)
def test_golden_files_by_windows(tool, tmp_path, name):
    d = open(os.path.join(GOLDEN, name), "rb").read()
    _check_all_windows(tool, tmp_path, d, (100, 4096, 65536, 1 << 20), want_broken=0)


def test_member_starts_around_window_starts(tool, tmp_path):
    members = [K.stored_member(K.text_stream(n)) for n in (100, 169, 1, 0, 500)] * 3
    d = b"".join(members) + K.EOF_BLOCK
    starts = [b[0] for b in K.chain_serial(d)]
    assert len(starts) == 16
    for s in starts[1:6]:
        for W in (s - 1, s, s + 1):  # window 1 starts one before, at, one after a member start
            _check_all_windows(tool, tmp_path, d, (W,), want_broken=0)
    # a member longer than the window: windows without any start
    _check_all_windows(tool, tmp_path, d, (26, 50, 131), want_broken=0)
    # sizes of one under, exactly and one over a multiple of the window
    for W in (len(d) - 1, len(d), len(d) + 1, (len(d) - 1) // 3):
        _check_all_windows(tool, tmp_path, d, (W,), want_broken=0)
    _check_all_windows(tool, tmp_path, K.stored_member(b"x\n"), (10, 64), want_broken=0)  # a single member
    _check_all_windows(tool, tmp_path, K.EOF_BLOCK, (10, 28, 64), want_broken=0)          # only the EOF block
    _check_all_windows(tool, tmp_path, b"", (64,), want_broken=0)


@pytest.mark.parametrize("fake", ["empty", "data", "two"])
def test_fake_member_is_a_windows_first_hit(tool, tmp_path, fake):
    """A complete member inside stored payload, first guesser hit of a window: the link to that
    window breaks and the repair gives the serial chain."""
    f1 = K.EOF_BLOCK if fake != "data" else K.deflated_member(b"hello, world")
    pay = b"a" * 40 + f1 + b"b" * 300 + (K.EOF_BLOCK if fake == "two" else b"") + b"c" * 50
    d = K.stored_member(b"x" * 10) + K.stored_member(pay) + K.stored_member(b"tail\n" * 30) + K.EOF_BLOCK
    at = d.find(f1, 30)
    assert K.guess_next(d, at, 1 << 40)[0] == at and at not in [b[0] for b in K.chain_serial(d)]
    want = _check_all_windows(tool, tmp_path, d, (at, at - 5), want_broken=1)
    assert len(want) == 4
    if fake == "two":  # two window starts in a row are fakes
        at2 = d.find(K.EOF_BLOCK, at + 28)
        W = at2 - at
        got, broken = run_chain(tool, tmp_path / "f.bin", W, at % W)
        assert broken == 1 and got == K.chain_serial(d, at % W)
    _check_all_windows(tool, tmp_path, d, (7, 100, 1000, len(d)))


def test_dense_members(tool, tmp_path):
    d = K.EOF_BLOCK * 2000 + K.stored_member(b"data\n" * 100) + K.EOF_BLOCK
    _check_all_windows(tool, tmp_path, d, (28, 29, 1000, 65536), want_broken=0)
    d = b"".join(K.deflated_member(K.text_stream(100, s)) for s in range(300)) + K.EOF_BLOCK
    _check_all_windows(tool, tmp_path, d, (64, 5000), want_broken=0)


def test_chain_ends_early(tool, tmp_path):
    good = [K.stored_member(K.text_stream(200, s)) for s in range(6)]
    # XLEN != 6 with a second subfield: the guesser takes it, htsjdk does not -- the chain ends there,
    # and the windows behind it are emptied
    odd = K.stored_member(b"odd\n", extra=b"XY\x02\x00\x07\x07")
    d = b"".join(good[:3]) + odd + b"".join(good[3:]) + K.EOF_BLOCK
    assert K.guess_next(d, 3 * len(good[0]), 1 << 40)[0] == 3 * len(good[0])
    want = _check_all_windows(tool, tmp_path, d, (50, 231, 400, 10000))
    assert len(want) == 3
    whole = b"".join(good)
    last = len(whole) - len(good[-1])
    for cut in list(range(last, last + 19)) + list(range(len(whole) - 9, len(whole))):  # header, trailer
        want = _check_all_windows(tool, tmp_path, whole[:cut], (100, 231, 5000))
        assert len(want) == 5
    _check_all_windows(tool, tmp_path, whole + K.EOF_BLOCK + b"garbage" * 9, (100, 5000))  # trailing garbage
    assert len(_check_all_windows(tool, tmp_path, whole, (100, 5000))) == 6               # no EOF block


def test_shard_chain_start(tool, tmp_path):
    members = [K.stored_member(K.text_stream(300, s)) for s in range(8)]
    d = b"".join(members) + K.EOF_BLOCK
    shard = d[100:-40]  # begins and ends inside a member
    start = K.first_guess(shard)
    assert start == len(members[0]) - 100
    want = _check_all_windows(tool, tmp_path, shard, (64, 331, 1000), start=start)
    assert len(want) == 6
    # a fake member in stored payload is the shard's first hit: the chain is that member alone
    pay = b"z" * 30 + K.EOF_BLOCK + b"y" * 200
    d2 = K.stored_member(b"h" * 50) + K.stored_member(pay) + K.stored_member(b"t\n" * 40) + K.EOF_BLOCK
    at = d2.find(K.EOF_BLOCK, 60)
    fake_first = d2[at - 7:]
    assert K.first_guess(fake_first) == 7
    assert len(_check_all_windows(tool, tmp_path, fake_first, (20, 64, 1000), start=7)) == 1
    none = d[100:len(members[0]) - 1]  # no hit at all: the chain starts at L and is empty
    assert K.first_guess(none) == len(none)
    assert _check_all_windows(tool, tmp_path, none, (64,), start=len(none)) == []


# ---------------------------------------------------------------- the planners' guess loop
def test_guess_over_ranges(tool, tmp_path):
    pay = b"q" * 20 + K.MAGIC + b"\x00" * 20 + K.EOF_BLOCK + b"r" * 2000
    d = K.stored_member(b"h" * 700) + K.stored_member(pay) + K.stored_member(b"t" * 900) + K.EOF_BLOCK
    f = tmp_path / "g.bin"
    f.write_bytes(d)
    L = len(d)
    for p in range(0, L, 37):
        for e in (p + 1, p + 600, L + 10):
            want = K.guess_next(d, p, e)
            assert run_guess(tool, f, p, e) == (want or "null"), (p, e)
            # a range that holds the answer (or runs to the split end, or to the end of the data)
            # gives the same answer; a shorter one says so and never takes a hit from elsewhere
            far = want[0] + 4 if want else min(e, L)
            assert run_guess(tool, f, p, e, [(p, far), (L - 10, L)]) == (want or "null"), (p, e)
            got = run_guess(tool, f, p, e, [(p, p + 8), (L - 40, L)])
            assert got in ("unknown", want or "null"), (p, e)
            if want and want[0] >= p + 8 and p + 8 < min(e, L - 3):
                assert got == "unknown", (p, e)
    assert run_guess(tool, f, 10, L, [(100, 200)]) == "unknown"  # p outside every range


def test_plain_build_agrees(tmp_path):
    """The unsanitized build gives the same table on a golden file."""
    exe = _build(tmp_path, "chain_check", ["-O2"])
    d = open(os.path.join(GOLDEN, "1.bam"), "rb").read()
    got, broken = run_chain(exe, os.path.join(GOLDEN, "1.bam"), 70000)
    assert got == K.chain_serial(d) and broken == 0
