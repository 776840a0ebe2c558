"""Aux tag decode benchmark (row f12): a synthetic BAM open on the device, the records stage run once,
then dq_tags_run's two passes (check, decode) timed with the records, their columns and the tag
columns resident in HBM.

  python tools/tags_bench.py [--gb 12.5] [--shape wgs|longread] [--steps 5] [--ab] [--out FILE]

--gb is the compressed size of the generated file (approximately; 12.5 is bench.py's input shape).
Per key list ([NM], [NM, AS, XS, RG], all six tags the generator writes) it reports the device ms of
the two passes (HIP events: dq_tags_run's ms_records less the records stage's, the median of --steps
runs after a warm-up), records/s, aux GB/s (the aux bytes, once), and the bytes the passes must touch
-- the aux bytes and the geometry columns (rec_lin, block_size, l_seq, n_cigar, l_read_name: 19 bytes
a record) twice, the tag columns once -- over the time as a fraction of the 8 TB/s HBM roof.  The
records stage's own time is quoted beside it.  --ab runs the two walk paths (the aux region copied
into the thread's LDS slot, and DQ_TAGS_STAGE=0: every record walked in memory) in turn, --steps
times each, interleaved in one process.  The CPU point: the same walk by tools/tags_check.cpp's code
(compiled here with g++ -O2) on 16 host threads over the records of the leading partitions (--cpu-mb
of them), as records/s.  Parity: the columns of a sample of partitions against tests/tagutil.py on the bytes
dq_decode exports for them."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ROOF = 8e12
GEOMETRY_BYTES = 8 + 4 + 4 + 2 + 1


def median(x):
    return sorted(x)[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=12.5, help="compressed GB of the file (approximately)")
    ap.add_argument("--shape", choices=("wgs", "longread"), default="wgs")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ab", action="store_true", help="the LDS slot against the memory walk, interleaved")
    ap.add_argument("--cpu-mb", type=int, default=512, help="MB of records the CPU baseline walks")
    ap.add_argument("--sample", type=int, default=4, help="partitions compared with tagutil")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401 -- one HIP runtime
    from disq_amd import _lib, synth
    import tagutil as U

    t0 = time.time()
    shape = {"wgs": synth.WGS, "longread": synth.LONGREAD}[a.shape]
    probe = synth.generate(20000 if a.shape == "wgs" else 500, seed=a.seed, shape=shape, nthreads=16)
    per_rec = len(probe.bam) / probe.n_records
    r = synth.generate(max(100, int(a.gb * 1e9 / per_rec)), seed=a.seed, shape=shape, nthreads=16)
    gen_s = time.time() - t0
    six = [("RG", U.STRING), ("NM", U.INT), ("MD", U.STRING), ("AS", U.INT), ("XS", U.INT), ("MC", U.STRING)]
    lists = {"NM": [("NM", U.INT)], "NM,AS,XS,RG": [("NM", U.INT), ("AS", U.INT), ("XS", U.INT), ("RG", U.STRING)],
             "RG,NM,MD,AS,XS,MC": six}
    os.environ.pop("DQ_TAGS_STAGE", None)
    out = {"metric": "aux tag decode, device ms of check + decode (row f12)", "unit": "ms", "steps": a.steps}
    with _lib.Context() as c:
        c.open_bytes(r.bam)
        base = c.run_resident()
        n = int(base.n_records)

        def tag_ms(keys):
            st = c.tags_run(keys)
            return st.ms_records - c.stats().ms_records

        results, ab = {}, {}
        for name, keys in lists.items():
            tag_ms(keys)  # warm-up: the columns grow to size
            ms = {m: [] for m in ((1, 0) if a.ab else (None,))}
            for _ in range(a.steps):
                for m in ms:
                    if m is not None:
                        os.environ["DQ_TAGS_STAGE"] = str(m)
                    ms[m].append(tag_ms(keys))
            os.environ.pop("DQ_TAGS_STAGE", None)
            if a.ab:
                ab[name] = {("slot" if m else "memory"): {"device_ms": round(median(v), 4),
                                                          "ms_all_runs": [round(x, 4) for x in v]}
                            for m, v in ms.items()}
            results[name] = [tag_ms(keys) for _ in range(a.steps)] if a.ab else ms[None]
        # the aux bytes, from the columns the records stage keeps
        b = c.read(with_raw=False)
        aux = int((4 + b["block_size"].astype(np.int64) - 36 - b["l_read_name"] - 4 * b["n_cigar"].astype(np.int64) -
                   (b["l_seq"].astype(np.int64) + 1) // 2 - b["l_seq"]).sum())
        rows = len(b["block_size"])
        po = b["part_offset"]
        del b
        g = c.tags(six)
        # parity on a sample of partitions: dq_decode's bytes of each through tagutil
        chunks = [ch for _, _, ch in c.plan() if ch is not None]
        ok, checked = len(chunks) == len(po) - 1, 0
        for p in sorted(set(np.linspace(0, len(chunks) - 1, num=min(a.sample, len(chunks)), dtype=int).tolist())):
            d = c.decode(chunks[p][0], chunks[p][1], with_raw=True)
            raw, ro, bs = d["raw"], d["raw_offset"], d["block_size"]
            recs = [bytes(raw[int(ro[i]):int(ro[i]) + 4 + int(bs[i])]) for i in range(len(bs))]
            lo, hi = int(po[p]), int(po[p + 1])
            cells, first = U.decode_records(recs, six)
            ok = ok and first is None and hi - lo == len(recs)
            if ok:
                want = U.want_arrays(cells, six)
                for k in ("flags", "vtype", "subtype", "val_off", "val_len"):
                    ok = ok and bool(np.array_equal(g[k][:, lo:hi], want[k]))
                for q in range(len(six)):
                    if want["key_base"][q] >= 0:
                        at, wt = int(g["key_base"][q]), int(want["key_base"][q])
                        ok = ok and bool(np.array_equal(g["val"][at + lo:at + hi], want["val"][wt:wt + len(recs)]))
            checked += len(recs)
        del g
        # the CPU baseline's records: the raw bytes of the leading partitions, up to --cpu-mb
        cpu_raw, got = [], 0
        for vs, ve in chunks:
            d = c.decode(vs, ve, with_raw=True)
            cpu_raw.append(np.array(d["raw"], copy=True))
            got += len(cpu_raw[-1])
            if got >= a.cpu_mb << 20:
                break
    out["records"], out["rows"], out["aux_bytes"] = n, rows, aux
    out["records_stage_ms"] = round(base.ms_records, 3)
    out["key_lists"] = {}
    for name, ms in results.items():
        keys = lists[name]
        med = median(ms)
        nval = sum(1 for _, t in keys if t in (U.INT, U.FLOAT, U.CHAR))
        touched = 2 * (aux + GEOMETRY_BYTES * rows) + rows * (11 * len(keys) + 4 * nval)
        out["key_lists"][name] = {
            "device_ms": round(med, 4), "ms_all_runs": [round(x, 4) for x in ms],
            "records_per_s": round(rows / (med / 1e3), 1), "aux_gb_per_s": round(aux / (med / 1e3) / 1e9, 2),
            "bytes_touched": touched, "hbm_roof_fraction": round(touched / (med / 1e3) / HBM_ROOF, 5)}
    out["value"] = out["key_lists"]["RG,NM,MD,AS,XS,MC"]["device_ms"]
    if a.ab:
        out["staging_ab"] = {"modes": "slot: the thread's aux region copied into its LDS slot; memory: every "
                                      "record walked in memory (DQ_TAGS_STAGE=0)",
                             "order": "slot, memory, slot, memory, ... in one process", "key_lists": ab}
    # the CPU point: 16 threads over a prefix of the records
    with tempfile.TemporaryDirectory() as tmp:
        exe, src = os.path.join(tmp, "tags_check"), os.path.join(tmp, "in.bin")
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "disq_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tools", "tags_check.cpp")], check=True)
        with open(src, "wb") as fh:
            for x in cpu_raw:
                x.tofile(fh)
        arg = ",".join(f"{k}:{t}" for k, t in six)
        cpu = json.loads(subprocess.run([exe, "bench", src, arg, "16", "3"], check=True,
                                        capture_output=True).stdout)
    out["cpu_16_threads"] = {"what": "tools/tags_check.cpp bench: check walk + decode walk, all six keys, best of 3",
                             "records": cpu["records"], "ms": cpu["ms_best"],
                             "records_per_s": round(cpu["records"] / (cpu["ms_best"] / 1e3), 1),
                             "bad_records": cpu["bad_records"]}
    out["config"] = {"compressed_gb": round(len(r.bam) / 1e9, 4), "inflated_gb": round(base.decompressed_bytes / 1e9, 4),
                     "mean_aux_bytes": round(aux / max(rows, 1), 1), "shape": a.shape,
                     "generator_s": round(gen_s, 1), "data": "synthetic BAM (seeded, %s shape)" % a.shape}
    out["parity"] = {"status": "match" if ok else "MISMATCH", "records": checked,
                     "checked": "the six keys' columns of a sample of partitions against tests/tagutil.py on "
                                "the bytes dq_decode exports for them"}
    text = json.dumps(out)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
