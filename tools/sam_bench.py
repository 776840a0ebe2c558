"""SAM text read path benchmark: a synthetic WGS-shaped BAM written out
as SAM text (tools/bam_to_sam.cpp, compiled here with g++), read by dq_sam_run with the text
resident: terminators, line table, partitions, size pass, encode pass, hashes and digests.

  python tools/sam_bench.py [--mb 1024] [--shape wgs|longread] [--split 33554432] [--steps 5]
                            [--prefix 2000] > out.json

--shape longread takes the generator's ONT-like reads (lines far over the 2 KB threshold, a wave
per line); --prefix is then better kept small (the Python oracle packs every base).

Reports GB/s of SAM text and records/s over the device time of dq_sam_run (HIP events, the median
of --steps runs after a warm-up) and, beside them, the time of the upload (dq_sam_open_memory:
host to device copy plus the host's header parse), which is not part of that figure.  Parity: the
first --prefix records' bytes equal tests/samutil.py's, and the whole file's per-partition counts
add up to its record lines."""
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


def make_sam(mb, seed, tmp, shape):
    """SAM text of about `mb` MB from a synthetic BAM: inflated on the device, written by the C++
    writer."""
    from disq_amd import _lib, synth
    exe = os.path.join(tmp, "bam_to_sam")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "bam_to_sam.cpp")],
                   check=True)
    shape = {"wgs": synth.WGS, "longread": synth.LONGREAD}[shape]
    probe = synth.generate(20000 if shape == synth.WGS else 500, seed=seed, shape=shape, nthreads=16)
    with _lib.Context() as c:
        c.open_bytes(probe.bam)
        per_rec = len(c.inflated()) * 1.25 / probe.n_records  # SAM text is about 1.25 x the BAM bytes
    n = max(100, int(mb * 1e6 / per_rec))
    r = synth.generate(n, seed=seed, shape=shape, nthreads=16)
    with _lib.Context() as c:
        c.open_bytes(r.bam)
        u = c.inflated()
    src, dst = os.path.join(tmp, "in.inflated"), os.path.join(tmp, "out.sam")
    u.tofile(src)
    subprocess.run([exe, src, dst], check=True)
    os.unlink(src)
    text = open(dst, "rb").read()
    os.unlink(dst)
    return text, r.n_records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="MB of SAM text (approximately)")
    ap.add_argument("--shape", choices=("wgs", "longread"), default="wgs")
    ap.add_argument("--split", type=int, default=32 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--prefix", type=int, default=2000, help="records compared with samutil")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch  # noqa: F401 -- one HIP runtime
    from disq_amd import _lib
    import samutil as S

    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        text, n_rec = make_sam(a.mb, a.seed, tmp, a.shape)
    gen_s = time.time() - t0
    with _lib.Context(split_size=a.split) as c:
        c.sam_open_bytes(text)  # warm-up of the upload path (buffers, pinned staging)
        w0 = time.perf_counter()
        c.sam_open_bytes(text)
        upload_ms = (time.perf_counter() - w0) * 1e3
        c.sam_run()  # warm-up: buffers grow to size
        ms = []
        for _ in range(a.steps):
            w0 = time.perf_counter()
            st = c.sam_run()
            ms.append((st.ms_total, st.ms_plan, st.ms_records, (time.perf_counter() - w0) * 1e3))
        cnt, _ = c.partition_digests()
    med = sorted(ms)[len(ms) // 2]
    # parity on a prefix: the text up to the end of its first --prefix record lines, read whole
    lines = S.text_lines(text[:min(len(text), (4 << 20) if a.shape == "wgs" else (24 << 20))])
    rec_lines = [(o, v) for o, v in lines[:-1] if not v.startswith(b"@")][:a.prefix]
    cut = rec_lines[-1][0] + len(rec_lines[-1][1]) + 1
    want = [r for _, _, r in S.sam_records(text[:cut])]
    with _lib.Context() as c:
        c.sam_open_bytes(text[:cut])
        b = c.sam_read(with_raw=True)
    raw, ro, bs = b["raw"], b["raw_offset"], b["block_size"]
    got = [bytes(raw[int(ro[i]):int(ro[i]) + 4 + int(bs[i])]) for i in range(len(bs))]
    ok = got == want and int(cnt.sum()) == n_rec == int(st.n_records)
    out = {
        "metric": "SAM text GB/s (SAM read path, row f7)",
        "value": round(len(text) / (med[0] / 1e3) / 1e9, 3), "unit": "GB/s",
        "device_ms": round(med[0], 3), "ms_lines_and_partitions": round(med[1], 3),
        "ms_records": round(med[2], 3), "wall_ms": round(med[3], 3), "steps": a.steps,
        "ms_all_runs": [round(m[0], 3) for m in ms],
        "records": int(st.n_records), "records_per_s": round(st.n_records / (med[0] / 1e3), 1),
        "upload_ms": round(upload_ms, 3),
        "config": {"sam_gb": round(len(text) / 1e9, 4), "split_size": a.split,
                   "partitions": int(st.n_partitions),
                   "mean_line_bytes": round(len(text) / max(int(st.n_records), 1), 1),
                   "generator_s": round(gen_s, 1),
                   "shape": a.shape,
                   "data": "synthetic BAM (seeded, %s shape) written as SAM text" % a.shape},
        "parity": {"status": "match" if ok else "MISMATCH", "prefix_records": len(want),
                   "checked": "record bytes of a prefix against tests/samutil.py; partition counts "
                              "of the whole file add up to its record lines"},
    }
    print(json.dumps(out), flush=True)
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
