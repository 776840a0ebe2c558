"""dqc::last_block_le (disq_amd/csrc/dq_chain_core.h) on the CPU through tools/block_range_check.cpp:
the split's last block by an upper-bound search of the block table, against the block-by-block loop
plan_blocks_kernel ran before (restated here in Python and, inside the tool, in C++).  The tool is
built with the sanitizers, so every case below is also a sanitizer run; a plain build is held
against it once."""
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disq_amd", "csrc")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-g", "-std=c++17", "-Wall", *flags, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "block_range_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("blockrange"), "block_range_check_san",
                  ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def linear(pos, j, e):
    """BgzfBlockSource's blocks of a split from block j: blocks while start <= split end."""
    jl = j
    while jl + 1 < len(pos) and pos[jl + 1] <= e:
        jl += 1
    return jl


def write_pos(path, pos):
    path.write_bytes(struct.pack(f"<{len(pos)}q", *pos))
    return path


def query(tool, path, pairs):
    out = subprocess.run([tool, "query", str(path), *[str(x) for p in pairs for x in p]], check=True,
                         stdout=subprocess.PIPE).stdout.decode().split("\n")
    return [tuple(map(int, l.split())) for l in out[:len(pairs)]]


def check(tool, path, pos, pairs):
    got = query(tool, path, pairs)
    assert len(got) == len(pairs)
    for (j, e), (search, lin) in zip(pairs, got):
        want = linear(pos, j, e)
        assert lin == want and search == want, (j, e, search, lin, want)


def sweep(tool, path, js):
    r = subprocess.run([tool, "sweep", str(path), *map(str, js)], stdout=subprocess.PIPE)
    cases, bad = map(int, r.stdout.decode().split())
    assert r.returncode == 0 and bad == 0, (cases, bad)
    return cases


POS = [0, 100, 250, 251, 900, 4000, 4028, 4056, 70000]  # 28-byte steps: empty members in a row


def test_split_end_around_block_positions(tool, tmp_path):
    f = write_pos(tmp_path / "p.bin", POS)
    pairs = []
    for j in range(len(POS)):
        for k in range(len(POS)):
            pairs += [(j, POS[k] - 1), (j, POS[k]), (j, POS[k] + 1)]  # one below, at, one above
    check(tool, f, POS, pairs)
    assert query(tool, f, [(2, 4028)])[0] == (6, 6) and query(tool, f, [(2, 4027)])[0] == (5, 5)


def test_split_end_before_the_next_block(tool, tmp_path):
    f = write_pos(tmp_path / "p.bin", POS)
    # e before block j + 1, down to before block j itself and before the table: never before j
    check(tool, f, POS, [(j, e) for j in range(len(POS)) for e in (POS[j], POS[j] - 1, POS[0] - 1, -5)])
    assert query(tool, f, [(3, 0)])[0] == (3, 3)


def test_split_end_past_the_last_block(tool, tmp_path):
    f = write_pos(tmp_path / "p.bin", POS)
    last = len(POS) - 1
    check(tool, f, POS, [(j, e) for j in range(len(POS)) for e in (POS[-1] + 1, 1 << 40, (1 << 62))])
    assert query(tool, f, [(0, 1 << 40)])[0] == (last, last)


def test_single_block_and_last_block(tool, tmp_path):
    one = [12345]
    f = write_pos(tmp_path / "one.bin", one)
    check(tool, f, one, [(0, e) for e in (0, 12344, 12345, 12346, 1 << 40)])
    assert sweep(tool, f, [0]) == 5
    g = write_pos(tmp_path / "p.bin", POS)
    last = len(POS) - 1
    check(tool, g, POS, [(last, e) for e in (0, POS[-1] - 1, POS[-1], POS[-1] + 1, 1 << 40)])  # j the last block


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 65, 1000, 4999, 5000])
def test_random_ascending_tables(tool, tmp_path, n):
    rng = random.Random(n)
    pos, p = [], rng.randrange(0, 1000)
    for _ in range(n):
        pos.append(p)
        p += rng.choice((1, 26, 28, 28, 500, 20000, 65536))
    f = write_pos(tmp_path / "r.bin", pos)
    js = sorted({0, 1 % n, n // 2, max(0, n - 2), n - 1, *(rng.randrange(n) for _ in range(3))})
    assert sweep(tool, f, js) == len(js) * (3 * n + 2)  # the tool's own loop, every edge of every block
    pairs = [(rng.randrange(n), rng.randrange(pos[0] - 2, pos[-1] + 3)) for _ in range(200)]
    check(tool, f, pos, pairs)  # and this file's loop on random split ends


def test_plain_build_agrees(tmp_path):
    exe = _build(tmp_path, "block_range_check", ["-O2"])
    f = write_pos(tmp_path / "p.bin", POS)
    check(exe, f, POS, [(j, e) for j in range(len(POS)) for e in range(-1, 4100, 7)])
