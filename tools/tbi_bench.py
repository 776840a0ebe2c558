"""GPU tabix index build (row f6, DESIGN.md "Building the .tbi"): the device time of
dq_text_write_tbi's index build on the synthetic VCFs of tools/vcf_bench.py (sites-only and 200
samples), beside the device time of dq_text_run over the same resident file.

  python tools/tbi_bench.py [--mb 1024] [--samples 0,200] [--reps 3] [--parity-mb 4] > out.json

Parity: on a file of --parity-mb from the same generator the index bytes equal the plain-Python
restatement of the rules (tests/tbiutil.py), and at full size the interval traversal through the
GPU-built index keeps every line that overlaps the seeded intervals (counted by the line filter
alone through an index of one whole-file chunk)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def whole_file_tabix(names, bgzf_len):
    import struct
    nm = b"".join(n + b"\x00" for n in names)
    d = b"TBI\x01" + struct.pack("<8i", len(names), 2, 1, 2, 0, ord("#"), 0, len(nm)) + nm
    for _ in names:
        d += struct.pack("<iIiQQi", 1, 0, 1, 0, bgzf_len << 16, 0)
    return d


def measure(_lib, vcf_bench, tbiutil, mb, samples, reps, parity_mb, procs, split):
    _, small = vcf_bench.make_vcf(parity_mb, samples, procs, tabix_range=True)
    with _lib.Context() as c:
        c.text_open_bytes(small)
        same = c.text_write_tbi() == tbiutil.build_tbi(small)
    _, data = vcf_bench.make_vcf(mb, samples, procs, tabix_range=True)
    rng = np.random.default_rng(3)
    with _lib.Context(split_size=split) as c:
        c.text_open_bytes(data)
        runs = []
        for _ in range(reps + 1):   # the first run warms up
            st = c.text_run(True)
            tbi = c.text_write_tbi()
            runs.append((c.tbi_ms, st.ms_total))
        names = tbiutil.parse_tbi(tbi)["names"]
        ivs = [(names[int(rng.integers(0, len(names)))].decode(), int(s), int(s + 10 ** rng.uniform(2, 5)))
               for s in rng.integers(1, 100_000_000, 200)]
        kept = {}
        for which, index in (("gpu", tbi), ("whole_file", whole_file_tabix(names, len(data)))):
            c.text_set_index(index)
            c.text_set_intervals(ivs)
            r = c.text_run(True)
            kept[which] = (int(r.n_records), int(r.n_partitions))
    med = sorted(runs[1:])[len(runs[1:]) // 2]
    ok = same and kept["gpu"][0] == kept["whole_file"][0]
    return {"samples": samples, "file_gb": round(len(data) / 1e9, 3),
            "decompressed_gb": round(st.decompressed_bytes / 1e9, 3), "lines": int(st.n_records),
            "contigs": len(names), "tbi_bytes": len(tbi), "tbi_ms": round(med[0], 3),
            "text_run_ms": round(med[1], 3), "tbi_ms_all_runs": [round(x[0], 3) for x in runs[1:]],
            "reps": reps,
            "parity": {"restatement_mb": parity_mb, "restatement": "match" if same else "MISMATCH",
                       "intervals": len(ivs), "kept": kept["gpu"][0],
                       "kept_whole_file_index": kept["whole_file"][0],
                       "partitions": kept["gpu"][1], "partitions_whole_file_index": kept["whole_file"][1],
                       "status": "match" if ok else "MISMATCH"}}, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="decompressed MB (approximately)")
    ap.add_argument("--samples", default="0,200")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parity-mb", type=int, default=4)
    ap.add_argument("--split", type=int, default=32 << 20)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    import torch  # noqa: F401 -- one HIP runtime
    from disq_amd import _lib
    import tbiutil
    import vcf_bench
    rows, good = [], True
    for s in (int(x) for x in a.samples.split(",")):
        row, ok = measure(_lib, vcf_bench, tbiutil, a.mb, s, a.reps, a.parity_mb, a.procs, a.split)
        rows.append(row)
        good = good and ok
    print(json.dumps({"metric": "device ms of the tabix index build (row f6)", "rows": rows}), flush=True)
    if not good:
        sys.exit(3)


if __name__ == "__main__":
    main()
