"""Instruction mix of the fused field-MLP kernels' chunk-pair loop on the compiled gfx950 ISA (CPU:
hipcc cross-compiles, nothing runs).  The 16-sample kernels of csrc/mlp_fused.hip are issue-bound
(DESIGN.md §3), so the instructions a 256 -> 256 layer's chunk pair carries beside its 48 MFMAs are
the quantity the plain-layer loop exists to cut.  tools/isa_pair.py finds that loop on the
control-flow graph and totals its instruction classes; this test
* pins the counter on a small synthetic listing (a rotated loop, a rarely taken side block, a
  second qualifying loop with more vector-memory instructions, a loop with the wrong MFMA count);
* compiles mlp_fused.hip as tests/test_isa_waits.py does and requires, for the forward
  (mlp_fused_kernel<0>) and the input-gradient chain (<1>), strictly fewer non-MFMA instructions
  per pair than the parent commit's loop had (profiles/plain01/isa_pair_counts.json, "parent"), no
  scratch and at most 256 VGPRs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf-experiments_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_pair as P  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["mlp_fused_kernelILi0E", "mlp_fused_kernelILi1E"]

SYNTH = """_Z6kernelILi0EEvv:
; %bb.0:
  s_load_dword s0, s[4:5], 0x0
  s_branch .LBB0_3
.LBB0_1:
  v_readlane_b32 s3, v9, 0
  s_mov_b32 s2, s3
.LBB0_2:
  v_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]
  v_add_f32_e32 v4, v5, v6
  s_add_i32 s1, s1, 2
  s_cmp_ge_i32 s1, s0
  s_cbranch_scc1 .LBB0_4
.LBB0_3:
  s_waitcnt vmcnt(1)
  s_barrier
  ds_read_b128 v[4:7], v12
  buffer_load_dwordx4 v13, s[8:11], s2 offen lds
  v_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]
  buffer_store_dwordx4 v[0:3], v14, s[8:11], 0 offen
  s_waitcnt vmcnt(3)
  s_barrier
  s_cmp_lt_i32 s6, 2
  s_cbranch_scc1 .LBB0_2
; %bb.5:
  s_add_i32 s6, s6, -1
  s_cmp_lg_u32 s6, 0
  s_cbranch_scc0 .LBB0_1
  s_branch .LBB0_2
.LBB0_4:
  s_mov_b32 s20, 0
.LBB0_6:
  s_barrier
  v_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]
  buffer_store_dwordx4 v[0:3], v14, s[8:11], 0 offen
  buffer_store_dwordx4 v[0:3], v14, s[8:11], 0 offen
  buffer_store_dwordx4 v[0:3], v14, s[8:11], 0 offen
  s_barrier
  v_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]
  s_add_i32 s20, s20, 1
  s_cmp_lt_i32 s20, s0
  s_cbranch_scc1 .LBB0_6
.LBB0_7:
  s_barrier
  v_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]
  s_barrier
  s_add_i32 s21, s21, 1
  s_cmp_lt_i32 s21, s0
  s_cbranch_scc1 .LBB0_7
  s_endpgm
.Lfunc_end0:
  .set _Z6kernelILi0EEvv.num_vgpr, 15
  .set _Z6kernelILi0EEvv.private_seg_size, 0
"""


def test_counter_on_a_synthetic_listing():
    # the first loop (header .LBB0_3, placed after its latch .LBB0_2, side block .LBB0_1 included):
    # 2 MFMA, 2 barriers, 2 vector-memory instructions; by hand: blocks .LBB0_1 (1 VALU, 1 SALU),
    # .LBB0_2 (1 VALU, 3 SALU), .LBB0_3 (6 SALU, 1 LDS, 2 VMEM), %bb.5 (4 SALU).  The loop at
    # .LBB0_6 also has 2 MFMA and 2 barriers but 3 vector-memory instructions; the loop at .LBB0_7
    # has one MFMA.
    r = P.pair_counts(SYNTH, "kernelILi0E", mfma_per_pair=(2,))
    assert r == {"mfma": 2, "valu": 2, "salu": 14, "lds": 1, "vmem": 2, "other": 0, "non_mfma": 19, "blocks": 4}, r
    assert P.resources(SYNTH, "kernelILi0E") == (15, 0)
    with pytest.raises(LookupError):
        P.pair_counts(SYNTH, "kernelILi0E", mfma_per_pair=(48,))
    assert [P.classify(x) for x in ("v_mfma_f32_16x16x32_bf16", "v_add_f32_e32", "s_nop", "ds_write_b64",
                                    "buffer_load_dwordx4", "global_load_dword")] == \
        ["mfma", "valu", "salu", "lds", "vmem", "vmem"]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "mlp_fused.s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(PKG, "csrc"), "--cuda-device-only", "-S", os.path.join(PKG, "csrc", "mlp_fused.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return open(out).read()


@pytest.mark.parametrize("sym", KERNELS)
def test_plain_pair_carries_fewer_instructions_than_the_parent(sym, listing):
    committed = json.load(open(os.path.join(ROOT, "profiles", "plain01", "isa_pair_counts.json")))
    parent = committed["parent"][sym]
    r = P.pair_counts(listing, sym)
    vgpr, scratch = P.resources(listing, sym)
    print(sym, r, "vgpr", vgpr, "scratch", scratch, "parent", parent)
    assert r["mfma"] == 48                                   # 2 chunks x 8 k-blocks x 3 bf16 products
    assert r["non_mfma"] < parent["non_mfma"], (r, parent)
    assert scratch == 0
    assert vgpr <= 256
