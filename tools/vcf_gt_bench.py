"""VCF genotype decode benchmark: the synthetic VCFs of
tools/vcf_bench.py with N genotype columns (zlib level 5, 65280-byte BGZF blocks), the resident file
decoded by dq_vcf_run and then by dq_vcf_genotypes_run -- the check and decode passes of
dq_vcf_gt.hip over the sample columns -- against the same per-cell rules (dq_vcf_gt_core.h) run by
16 host threads (tools/vcf_gt_check.cpp, bench mode, one run of whole lines per thread).

  python tools/vcf_gt_bench.py [--mb 1024] [--samples 200] [--split 33554432] [--steps 5] > out.json

Reports the device time of the two genotype passes (HIP events: dq_vcf_genotypes_run's ms_records
less dq_vcf_run's) and the GB/s of decompressed text that is, beside dq_vcf_run of the same resident
file, the bytes of the matrix, the host baseline, and parity: every cell of every array equals the
host run's.  Synthetic data: no network for real VCFs."""
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


def median(v):
    return sorted(v)[len(v) // 2]


def read_matrix(path):
    """OUT.bin of `vcf_gt_check bench`."""
    with open(path, "rb") as fh:
        n, S, P = (int(x) for x in np.frombuffer(fh.read(24), "<i8"))
        c = n * S
        out = {"flags": np.frombuffer(fh.read(c), np.uint8).reshape(n, S),
               "ploidy": np.frombuffer(fh.read(c), np.uint8).reshape(n, S),
               "allele": np.frombuffer(fh.read(2 * c * P), "<i2").reshape(n, S, P)}
        for k in ("gq", "dp", "cell_off"):
            out[k] = np.frombuffer(fh.read(4 * c), "<i4").reshape(n, S)
    return out, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="decompressed MB (approximately)")
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--split", type=int, default=32 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    if a.samples < 1:
        ap.error("--samples: at least 1 (a sites-only file has no genotype matrix)")
    import torch  # noqa: F401 -- one HIP runtime
    import vcf_bench
    from disq_amd import _lib

    t0 = time.time()
    text, data = vcf_bench.make_vcf(a.mb, a.samples, a.procs, tabix_range=True)
    gen_s = time.time() - t0
    with _lib.Context(split_size=a.split, verify_crc=True) as c:
        c.text_open_bytes(data)
        c.vcf_run()
        c.vcf_genotypes_run()  # warm-up: buffers grow to size
        vms, gms = [], []
        for _ in range(a.steps):
            v = c.vcf_run()                # re-runs the text pipeline and the site passes
            g = c.vcf_genotypes_run()      # the genotype passes over the new run's columns
            vms.append((v.ms_total, v.ms_records))
            gms.append(g.ms_records - v.ms_records)
        w0 = time.perf_counter()
        m = c.vcf_genotypes()
        read_wall = time.perf_counter() - w0
    ubytes = v.decompressed_bytes
    dev, site = median([x[0] for x in vms]), median([x[1] for x in vms])
    gt = median(gms)
    n, S, P = m["flags"].shape[0], m["n_samples"], m["max_ploidy"]
    cell_bytes = 2 + 2 * P + 12
    with tempfile.TemporaryDirectory() as tmp:
        exe, src, dst = (os.path.join(tmp, x) for x in ("vcf_gt_check", "in.vcf", "out.bin"))
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "disq_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tools", "vcf_gt_check.cpp")], check=True)
        with open(src, "wb") as fh:
            fh.write(text)
        cpu = json.loads(subprocess.run([exe, "bench", src, str(a.threads), "3", dst], check=True,
                                        capture_output=True).stdout)
        host, hp = read_matrix(dst)
    bad = [k for k in host if host[k].shape != m[k].shape or not np.array_equal(host[k], m[k])]
    if hp != P or cpu["bad_lines"] or cpu["n_gq_host"] != m["n_gq_host"]:
        bad.append("scalars")
    out = {
        "metric": "decompressed VCF GB/s through the genotype passes alone (dq_vcf_genotypes_run less dq_vcf_run, row f10)",
        "value": round(ubytes / (gt / 1e3) / 1e9, 3), "unit": "GB/s",
        "genotype_passes_ms": round(gt, 3), "steps": a.steps,
        "cells": n * S, "cells_per_s": round(n * S / (gt / 1e3), 1),
        "matrix_bytes": n * S * cell_bytes, "matrix_bytes_per_cell": cell_bytes,
        "matrix_write_gb_s": round(n * S * cell_bytes / (gt / 1e3) / 1e9, 3),
        "vcf_run_device_ms": round(dev, 3), "vcf_run_validate_decode_ms": round(site, 3),
        "vcf_run_gb_s": round(ubytes / (dev / 1e3) / 1e9, 3),
        "genotypes_share_of_run": round(gt / (dev + gt), 4),
        "n_gq_host": m["n_gq_host"], "matrix_read_wall_s": round(read_wall, 3),
        "config": {"samples": S, "max_ploidy": P, "variants": n, "decompressed_gb": round(ubytes / 1e9, 4),
                   "compressed_gb": round(len(data) / 1e9, 4), "split_size": a.split,
                   "partitions": len(m["part_offset"]) - 1, "mean_line_bytes": round(ubytes / max(n, 1), 1),
                   "generator_s": round(gen_s, 1),
                   "data": "synthetic VCF (seeded), zlib level 5 BGZF, htsjdk block size"},
        "cpu_baseline": {"value": round(cpu["bytes"] / (cpu["ms_best"] / 1e3) / 1e9, 4), "unit": "GB/s",
                         "ms": cpu["ms_best"], "threads": cpu["threads"], "kind": "port",
                         "what": "dq_vcf_gt_core.h's check and decode walks over the uncompressed text in memory, "
                                 "one run of whole lines per thread, best of 3 (no inflate, no line splitting, "
                                 "no site decode)"},
        "parity": {"status": "match" if not bad else "MISMATCH", "bad_arrays": bad,
                   "checked": "every cell of flags, ploidy, allele, gq, dp and cell_off, max_ploidy and "
                              "n_gq_host, GPU vs the host run of the same rules"},
    }
    print(json.dumps(out), flush=True)
    if bad:
        sys.exit(3)


if __name__ == "__main__":
    main()
