"""The listing of csrc/mlp_rows_f2.hip, read the way tests/test_host_logic.py reads the other ring kernels': no kernel
may spill to scratch (a reload waits vmcnt(0) and drains the ring's prefetches), and no vector-memory instruction
inside an asm block may read an SGPR that a VALU instruction wrote fewer than five wait states earlier
(scripts/dev/scan_asm_hazards.py)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mlp_rows_f2ring_listing_has_no_scratch_and_no_asm_hazard(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
    try:
        import scan_asm_hazards
    finally:
        sys.path.pop(0)
    out = str(tmp_path / "mlp_rows_f2.s")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
           "-Wno-unused-function", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
           os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "mlp_rows_f2.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(scratch) == 12 and not any(scratch), scratch          # 3 depths x (decoder + 3 table formats of the encoder)
    occupancy = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert occupancy and min(occupancy) >= 2, occupancy              # 512 threads: two waves per SIMD must fit
    assert scan_asm_hazards.scan(out) == []
    assert scan_asm_hazards.scan_store_hazard(out) == []
