"""bench.py's file handling around the timed steps (no GPU): the --dump-outputs arrays, the input
slot that spares a run the file's generation, and the options of a plain run."""
import os
import sys

import numpy as np
import pytest

import bench


def test_dump_outputs_is_float64_and_exact(tmp_path):
    counts = np.array([295332, 0, 7], np.int64)
    digests = np.array([0xFFFFFFFFFFFFFFFF, 0, 0x0123456789ABCDEF], np.uint64)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), counts, digests, 35682089237, 109964499, 0x47DAB2473E7A4573)
    got = {n: np.load(out / n) for n in sorted(os.listdir(out))}
    assert sorted(got) == ["file_totals.npy", "partition_digests.npy", "partition_records.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["partition_records.npy"], counts)
    limbs = got["partition_digests.npy"]
    assert limbs.shape == (3, 4) and limbs.max() <= 0xFFFF
    back = sum(limbs[:, i].astype(np.uint64) << np.uint64(48 - 16 * i) for i in range(4))
    assert np.array_equal(back, digests)
    tot = got["file_totals.npy"]
    assert tot[0] == 35682089237 and tot[1] == 109964499
    assert [int(x) for x in tot[2:]] == [0x47DA, 0xB247, 0x3E7A, 0x4573]


def test_input_slot_round_trip(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "INPUT_DIR", str(tmp_path / "slot"))
    key = {"shape": "wgs", "gb": 0.001, "seed": 1, "records": 10}
    assert bench.load_input(key, True, 3) is None  # no slot yet
    data = np.random.default_rng(5).integers(0, 256, size=1_000_003, dtype=np.uint8)
    bench.store_input(key, data, b"BAI\x01")
    assert bench.slot_matches(key)
    buf, bai = bench.load_input(key, True, 3)  # 3 threads over a length they do not divide
    assert np.array_equal(buf, data) and buf.flags.writeable and bai == b"BAI\x01"
    assert bench.load_input(key, False, 16)[1] is None
    assert bench.load_input(dict(key, seed=2), True, 3) is None  # another file's key
    os.unlink(os.path.join(bench.INPUT_DIR, "key.json"))  # a half-written slot has no key yet
    assert bench.load_input(key, True, 3) is None


def test_input_key_follows_the_arguments(monkeypatch):
    def key(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return bench.input_key(bench.parse(), 1000)
    base = key()
    assert base == key("--steps", "9", "--full")  # the file does not depend on these
    assert base != key("--seed", "2") and base != key("--gb", "1") and base != key("--shape", "longread")


def test_plain_run_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
