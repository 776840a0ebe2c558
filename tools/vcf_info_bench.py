"""VCF INFO decode benchmark: the synthetic VCFs of
tools/vcf_bench.py (zlib level 5, 65280-byte BGZF blocks; sites-only, or N genotype columns), the
resident file decoded by dq_vcf_run and then by dq_vcf_info_run -- the check and decode passes of
dq_vcf_info.hip over the INFO column -- for 1, 4 and 12 requested keys, against the same per-line
rules (dq_vcf_info_core.h) run by 16 host threads (tools/vcf_info_check.cpp, bench mode, one run of
whole lines per thread).

  python tools/vcf_info_bench.py [--mb 1024] [--samples 0] [--split 33554432] [--steps 5] > out.json
  python tools/vcf_info_bench.py --mb 64 --pad 600 --ab      # both walks on INFO columns of 600 bytes

The generator's INFO column holds eight keys (AC AF AN DP FS MQ QD SOR, all typed Float by its
header); AC, AN and DP are asked for as Integer, and the list of 12 adds four keys no line holds.
Per key list it reports the device time of the two INFO passes (HIP events: dq_vcf_info_run's
ms_records less dq_vcf_run's) and the GB/s of decompressed text that is, beside dq_vcf_run of the
same resident file, the host baseline, and parity: every array equals the host run's.

--pad N (sites-only files) lengthens every INFO column to about N bytes with an annotation piece
nobody asks for; --ab runs every key list in two fresh processes, one sending every variant down
the thread walk and one down the wave walk (DQ_INFO_WAVE), which is how the threshold INFO_WAVE of
dq_vcf_info.hip is measured.  Synthetic data: no network for real VCFs."""
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

INT = 2
KEYS12 = [("DP", INT), "AF", "MQ", "QD", ("AC", INT), ("AN", INT), "FS", "SOR", "DB", "END", "SB", "AA"]
KEY_LISTS = {1: KEYS12[:1], 4: KEYS12[:4], 12: KEYS12}


def median(v):
    return sorted(v)[len(v) // 2]


def key_arg(keys):
    return ",".join(k if isinstance(k, str) else "%s:%d" % k for k in keys)


def read_columns(path):
    """OUT.bin of `vcf_info_check bench`."""
    b = np.fromfile(path, np.uint8)
    n, K, ni, nf, nhost = (int(x) for x in b[:40].view("<i8"))
    at = [40]

    def take(dt, count):
        a = b[at[0]:at[0] + count * np.dtype(dt).itemsize].view(dt)
        at[0] += a.nbytes
        return a
    g = {"key_type": take("<i4", K), "key_width": take("<i4", K), "key_base": take("<i8", K),
         "flags": take(np.uint8, K * n).reshape(K, n)}
    for k in ("n_values", "val_off", "val_len"):
        g[k] = take("<i4", K * n).reshape(K, n)
    g["ival"], g["fval"] = take("<i4", ni), take("<u8", nf)
    return g, nhost


def pad_info(text, pad, procs):
    """Every data line's INFO column (the last one: sites-only) brought to about `pad` bytes, and
    the BGZF of that text."""
    import vcf_bench
    from multiprocessing import Pool
    lines = text.split(b"\n")
    fill = b";CSQ=" + b"A|missense_variant|ENST00000|c.1A>T," * (pad // 30 + 1)
    out = [l if not l or l.startswith(b"#") else l + fill[:max(0, pad - (len(l) - l.rfind(b"\t") - 1))].rstrip(b",;")
           for l in lines]
    text = b"\n".join(out)
    vcf_bench._TEXT = text
    step = vcf_bench.BLOCK_U * 64
    with Pool(procs) as p:
        parts = p.map(vcf_bench._compress_job, [(a, min(a + step, len(text))) for a in range(0, len(text), step)])
    vcf_bench._TEXT = b""
    return text, b"".join(parts) + vcf_bench.EOF_BLOCK


def measure(data, split, steps, lists, want_columns):
    """Per key list: the INFO passes' and dq_vcf_run's device times; the columns when asked for."""
    import torch  # noqa: F401 -- one HIP runtime
    from disq_amd import _lib
    res = {}
    with _lib.Context(split_size=split, verify_crc=True) as c:
        c.text_open_bytes(data)
        for nk in lists:
            keys = KEY_LISTS[nk]
            c.vcf_run()
            c.vcf_info_run(keys)  # warm-up: buffers grow to size
            vms, ims = [], []
            for _ in range(steps):
                v = c.vcf_run()               # re-runs the text pipeline and the site passes
                i = c.vcf_info_run(keys)      # the INFO passes over the new run's columns
                vms.append((v.ms_total, v.ms_records))
                ims.append(i.ms_records - v.ms_records)
            r = {"info_passes_ms": round(median(ims), 3), "info_passes_ms_min_max": [round(min(ims), 3), round(max(ims), 3)],
                 "vcf_run_device_ms": round(median([x[0] for x in vms]), 3),
                 "vcf_run_validate_decode_ms": round(median([x[1] for x in vms]), 3),
                 "decompressed_bytes": int(v.decompressed_bytes)}
            if want_columns:
                w0 = time.perf_counter()
                r["columns"] = c.vcf_info(keys)
                r["read_wall_s"] = round(time.perf_counter() - w0, 3)
            res[nk] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024, help="decompressed MB (approximately, before --pad)")
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--split", type=int, default=32 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--pad", type=int, default=0, help="INFO columns of about this many bytes (sites-only)")
    ap.add_argument("--ab", action="store_true", help="thread walk against wave walk, a process each")
    ap.add_argument("--keys", type=int, nargs="*", default=[1, 4, 12], choices=[1, 4, 12])
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:  # one walk of --ab: the file is on disk, the times go to stdout
        data = open(a.child, "rb").read()
        print(json.dumps(measure(data, a.split, a.steps, a.keys, False)), flush=True)
        return
    if a.pad and a.samples:
        ap.error("--pad: sites-only files (INFO is the last column)")
    import vcf_bench

    t0 = time.time()
    text, data = vcf_bench.make_vcf(a.mb, a.samples, a.procs, tabix_range=True)
    if a.pad:
        text, data = pad_info(text, a.pad, a.procs)
    gen_s = time.time() - t0
    res = measure(data, a.split, a.steps, a.keys, True)
    n = res[a.keys[0]]["columns"]["flags"].shape[1]
    ubytes = res[a.keys[0]]["decompressed_bytes"]
    with tempfile.TemporaryDirectory() as tmp:
        exe, src, dst, bgz = (os.path.join(tmp, x) for x in ("vcf_info_check", "in.vcf", "out.bin", "in.vcf.bgz"))
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "disq_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tools", "vcf_info_check.cpp")], check=True)
        with open(src, "wb") as fh:
            fh.write(text)
        runs = []
        for nk in a.keys:
            r = res[nk]
            m = r.pop("columns")
            cpu = json.loads(subprocess.run([exe, "bench", src, key_arg(KEY_LISTS[nk]), str(a.threads), "3", dst],
                                            check=True, capture_output=True).stdout)
            host, nhost = read_columns(dst)
            bad = [k for k in host if host[k].shape != (m[k].view(np.uint64) if k == "fval" else m[k]).shape or
                   not np.array_equal(host[k], m[k].view(np.uint64) if k == "fval" else m[k])]
            if cpu["bad_lines"] or nhost != m["n_float_host"] or cpu["lines"] != n:
                bad.append("scalars")
            ms = r["info_passes_ms"]
            col_bytes = 13 * len(KEY_LISTS[nk]) * n + 4 * len(m["ival"]) + 8 * len(m["fval"])
            runs.append({"keys": nk, "key_list": key_arg(KEY_LISTS[nk]), **r,
                         "gb_s_of_text": round(ubytes / (ms / 1e3) / 1e9, 3),
                         "variants_per_s": round(n / (ms / 1e3), 1),
                         "column_bytes": col_bytes, "column_write_gb_s": round(col_bytes / (ms / 1e3) / 1e9, 3),
                         "n_float_host": m["n_float_host"], "key_width_max": int(m["key_width"].max()),
                         "cpu_baseline": {"ms": cpu["ms_best"], "threads": cpu["threads"], "kind": "port",
                                          "value": round(cpu["bytes"] / (cpu["ms_best"] / 1e3) / 1e9, 4), "unit": "GB/s"},
                         "parity": {"status": "match" if not bad else "MISMATCH", "bad_arrays": bad}})
        ab = None
        if a.ab:
            with open(bgz, "wb") as fh:
                fh.write(data)
            ab = {}
            for name, at in (("thread_walk", "2147483647"), ("wave_walk", "0")):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", bgz, "--split", str(a.split),
                       "--steps", str(a.steps), "--keys", *[str(k) for k in a.keys]]
                o = subprocess.run(cmd, check=True, capture_output=True, env=dict(os.environ, DQ_INFO_WAVE=at)).stdout
                ab[name] = {k: v["info_passes_ms"] for k, v in json.loads(o).items()}
    lines = [l for l in text[:1 << 20].split(b"\n") if l and not l.startswith(b"#")][:-1]
    info_len = [len(l.split(b"\t")[7]) for l in lines]
    bad = [r["keys"] for r in runs if r["parity"]["status"] != "match"]
    out = {
        "metric": "decompressed VCF GB/s through the INFO passes alone (dq_vcf_info_run less dq_vcf_run, row f11)",
        "value": runs[-1]["gb_s_of_text"], "unit": "GB/s", "value_keys": runs[-1]["keys"], "steps": a.steps,
        "runs": runs, "thread_against_wave_ms": ab,
        "config": {"samples": a.samples, "pad": a.pad, "variants": n, "decompressed_gb": round(ubytes / 1e9, 4),
                   "compressed_gb": round(len(data) / 1e9, 4), "split_size": a.split,
                   "mean_line_bytes": round(ubytes / max(n, 1), 1),
                   "mean_info_bytes": round(sum(info_len) / max(1, len(info_len)), 1),
                   "generator_s": round(gen_s, 1),
                   "data": "synthetic VCF (seeded), zlib level 5 BGZF, htsjdk block size"},
        "cpu_baseline_what": "dq_vcf_info_core.h's check and decode walks over the uncompressed text in memory, one run "
                             "of whole lines per thread, best of 3 (no inflate, no line splitting, no site decode)",
        "parity": {"status": "match" if not bad else "MISMATCH", "bad_key_lists": bad,
                   "checked": "every element of flags, n_values, val_off, val_len, ival, fval (bits), key_type, "
                              "key_width, key_base and n_float_host, GPU vs the host run of the same rules"},
    }
    print(json.dumps(out), flush=True)
    if bad:
        sys.exit(3)


if __name__ == "__main__":
    main()
