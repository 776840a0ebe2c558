"""VCF site decode benchmark: the synthetic VCFs of tools/vcf_bench.py
(zlib level 5, 65280-byte BGZF blocks; sites-only, or N genotype columns) read by dq_vcf_run -- the
text run of row f4, then the validate and decode passes of dq_vcf.hip -- against dq_text_run on the
same build and against the same per-line rules (dq_vcf_core.h) run by 16 host threads
(tools/vcf_core_check.cpp, bench mode, one run of whole lines per thread).

  python tools/vcf_decode_bench.py [--mb 1024] [--samples 0] [--split 33554432] [--steps 5] > out.json

Reports the device time of dq_vcf_run (HIP events) and the validate + decode share of it, the
device time of dq_text_run, the bytes a LINES and a SITES export move to the host, the host
baseline, and parity: every partition's columns equal the host run's.  Synthetic data: no network
for real VCFs.  The positions restart on every contig (vcf_bench's tabix_range files): numbered
through the whole file they pass 2^31 - 1 after 6 M lines, which VCFCodec.decode and dq_vcf_run
both refuse (POS)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROW = np.dtype([("contig", "<i4"), ("pos", "<i4"), ("end", "<i4"), ("flags", "<u4"), ("qual", "<f8"),
                ("col_end", "<i4", (8,)), ("n_alt", "<i4"), ("n_filter", "<i4"), ("n_info", "<i4"),
                ("n_sample_cols", "<i4")])
COLUMN_BYTES = 8 + 4 + 8 + ROW.itemsize  # line_offset, line_len, hash and the columns, per variant


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="decompressed MB (approximately)")
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--split", type=int, default=32 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    import torch  # noqa: F401 -- one HIP runtime
    import vcf_bench
    from disq_amd import _lib

    t0 = time.time()
    text, data = vcf_bench.make_vcf(a.mb, a.samples, a.procs, tabix_range=True)
    gen_s = time.time() - t0
    with _lib.Context(split_size=a.split, verify_crc=True) as c:
        c.text_open_bytes(data)
        c.vcf_run()  # warm-up: buffers grow to size
        vms, tms = [], []
        for _ in range(a.steps):
            st = c.vcf_run()
            vms.append((st.ms_total, st.ms_records))
        for _ in range(a.steps):
            tms.append(c.text_run(True).ms_total)
        w0 = time.perf_counter()
        sites = c.vcf_read(_lib.VCF_EXPORT_SITES)
        sites_wall = time.perf_counter() - w0
        w0 = time.perf_counter()
        lines = c.vcf_read(_lib.VCF_EXPORT_LINES)
        lines_wall = time.perf_counter() - w0
    dev = median([m[0] for m in vms])
    dec = median([m[1] for m in vms])
    tdev = median(tms)
    n = len(sites["pos"])
    ubytes = st.decompressed_bytes
    lines_bytes, sites_bytes = lines["n_bytes"], sites["n_bytes"]
    del lines
    # the host baseline and the parity reference: dq_vcf_core.h on `threads` host threads
    with tempfile.TemporaryDirectory() as tmp:
        exe, src, dst = (os.path.join(tmp, x) for x in ("vcf_core_check", "in.vcf", "out.bin"))
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "disq_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tools", "vcf_core_check.cpp")], check=True)
        with open(src, "wb") as fh:
            fh.write(text)
        cpu = json.loads(subprocess.run([exe, "bench", src, str(a.threads), "3", dst], check=True,
                                        capture_output=True).stdout)
        rows = np.fromfile(dst, ROW)
    bad = 0
    po = sites["part_offset"]
    if len(rows) != n or cpu["bad_lines"]:
        bad = len(po) - 1
    else:
        for p in range(len(po) - 1):
            lo, hi = int(po[p]), int(po[p + 1])
            same = all(np.array_equal(sites[k][lo:hi], rows[k][lo:hi]) for k in ROW.names if k != "qual")
            same = same and np.array_equal(sites["qual"][lo:hi].view(np.uint64), rows["qual"][lo:hi].view(np.uint64))
            bad += not same
    out = {
        "metric": "decompressed VCF GB/s, lines decoded into site columns (dq_vcf_run, row f9)",
        "value": round(ubytes / (dev / 1e3) / 1e9, 3), "unit": "GB/s",
        "device_ms": round(dev, 3), "validate_decode_ms": round(dec, 3),
        "validate_decode_share": round(dec / dev, 4), "text_run_device_ms": round(tdev, 3),
        "text_run_gb_s": round(ubytes / (tdev / 1e3) / 1e9, 3), "steps": a.steps,
        "variants": n, "variants_per_s": round(n / (dev / 1e3), 1),
        "validate_decode_gb_s": round(ubytes / (dec / 1e3) / 1e9, 3),
        "n_qual_host": sites["n_qual_host"],
        "d2h": {"lines_bytes": int(lines_bytes) + COLUMN_BYTES * n, "sites_bytes": int(sites_bytes) + COLUMN_BYTES * n,
                "lines_data_bytes": int(lines_bytes), "sites_data_bytes": int(sites_bytes),
                "column_bytes_per_variant": COLUMN_BYTES,
                "ratio": round((lines_bytes + COLUMN_BYTES * n) / max(1, sites_bytes + COLUMN_BYTES * n), 2),
                "lines_read_wall_s": round(lines_wall, 3), "sites_read_wall_s": round(sites_wall, 3)},
        "config": {"samples": a.samples, "decompressed_gb": round(ubytes / 1e9, 4),
                   "compressed_gb": round(len(data) / 1e9, 4), "split_size": a.split,
                   "partitions": len(po) - 1, "mean_line_bytes": round(ubytes / max(n, 1), 1),
                   "generator_s": round(gen_s, 1),
                   "data": "synthetic VCF (seeded), zlib level 5 BGZF, htsjdk block size"},
        "cpu_baseline": {"value": round(cpu["bytes"] / (cpu["ms_best"] / 1e3) / 1e9, 4), "unit": "GB/s",
                         "ms": cpu["ms_best"], "threads": cpu["threads"], "kind": "port",
                         "what": "dq_vcf_core.h's walk over the uncompressed text in memory, one run of whole "
                                 "lines per thread, best of 3 (no inflate, no line splitting)"},
        "parity": {"status": "match" if bad == 0 else "MISMATCH", "partitions": len(po) - 1,
                   "bad_partitions": int(bad),
                   "checked": "per-partition columns (contig, pos, end, flags, qual bits, col_end, counts), "
                              "GPU vs the host run of the same rules"},
    }
    print(json.dumps(out), flush=True)
    if bad:
        sys.exit(3)


if __name__ == "__main__":
    main()
