#!/bin/bash
# The device bounds-checked build (make -C disq_amd/csrc checked, -DDQ_CHECKED): the inflate,
# parity and adversarial GPU tests under libdisq_gpu_checked.so; the session fails on any failed
# device check (tests/conftest.py).  usage: tools/gpu_checked_tests.sh TAG [test files]
# (default: the inflate, parity, adversarial, chunk, text, deflate, hand-off, resolve-group,
# resolve-round, .bai, .tbi, SAM, header pre-pass, record-edge, coordinate-edge, batched-speculation
# and plan-edge tests)
set -eo pipefail
tag=$1
shift
tests=${@:-tests/test_inflate_codes.py tests/test_gpu_parity.py tests/test_adversarial.py tests/test_chunk_decode.py tests/test_text_gpu.py tests/test_deflate_gpu.py tests/test_tail_handoff.py tests/test_resolve_groups.py tests/test_resolve_rounds.py tests/test_bai.py tests/test_tbi.py tests/test_sam_gpu.py tests/test_header_prepass.py tests/test_header_prepass_counts.py tests/test_record_edges.py tests/test_coord_edges.py tests/test_spec_batched.py tests/test_plan_edges_gpu.py}
out=gpurun_out/$tag
mkdir -p $out
export TMPDIR=/tmp DQ_GPU_LIB=$PWD/disq_amd/_build/libdisq_gpu_checked.so
timeout -k 10 900 python3 -u -m pytest $tests \
  -m gpu -v -s --timeout 300 --timeout-method thread > $out/checked_tests.log 2>&1 || { tail -40 $out/checked_tests.log; exit 1; }
grep -h "DQ_CHECKED\|passed\|failed" $out/checked_tests.log | tail -3
