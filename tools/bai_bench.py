"""GPU .bai index build (row f5): the device time of dq_write_bai's index
build on a synthetic WGS-shaped BAM, beside the records stage and the whole pipeline of the same
(indexer-mode) run.

  python tools/bai_bench.py [--gb 2] [--reps 3] [--intervals 1000] > out.json

Parity at scale: for the seeded intervals, dq_run_resident's kept count and per-partition
(count, digest) with the GPU-built index equal those with the index the generator wrote while it
produced the file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=2.0, help="compressed GB of the generated file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--intervals", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch  # noqa: F401 -- one HIP runtime
    from disq_amd import _lib, synth
    probe = synth.generate(20000, seed=a.seed, nthreads=16)
    n = int(a.gb * 1e9 / (len(probe.bam) / probe.n_records))
    r = synth.generate(n, seed=a.seed, nthreads=16, bai=True)
    # intervals over the stretch of chr1 the records cover (5 b per record), lengths log-uniform
    # 100 b - 100 kb
    rng = np.random.default_rng(3)
    span = max(1000, 5 * n)
    ivs = [(0, int(s), int(s + 10 ** rng.uniform(2, 5))) for s in rng.integers(1, span, a.intervals)]
    with _lib.Context() as c:
        c.open_bytes(r.bam)
        runs = []
        for _ in range(a.reps + 1):   # the first run warms up
            bai, ms = c.write_bai_timed()
            st = c.stats()
            runs.append((ms, st.ms_records, st.ms_total))
        res = {}
        for name, index in (("gpu", bai), ("generator", r.bai)):
            c.set_index(index)
            st = c.run_resident((ivs, False))
            cnt, dig = c.partition_digests()
            res[name] = (int(st.n_filtered), int(st.blocks_inflated), cnt.copy(), dig.copy())
    g, w = res["gpu"], res["generator"]
    ok = g[0] == w[0] and np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3])
    med = sorted(runs[1:])[len(runs[1:]) // 2]
    out = {"file_gb": round(len(r.bam) / 1e9, 3), "records": r.n_records, "bai_bytes": len(bai),
           "ms": round(med[0], 3), "ms_records": round(med[1], 3), "ms_total": round(med[2], 3),
           "ms_all_runs": [round(x[0], 3) for x in runs[1:]], "reps": a.reps,
           "parity": {"intervals": len(ivs), "kept": g[0], "kept_generator_index": w[0],
                      "blocks_inflated": g[1], "blocks_inflated_generator_index": w[1],
                      "partitions": int(len(g[2])), "status": "match" if ok else "MISMATCH"}}
    print(json.dumps(out), flush=True)
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
