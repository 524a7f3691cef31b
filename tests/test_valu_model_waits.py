"""The scalar load / wait report of tools/valu_model.py (`scalar_load_waits`) on two step loops written by hand in the shape of
the compiler's listings: one that waits for its load at once, at the loop top, and one rotated by a step, whose load is covered
by a wait a loop body later. No compiler involved."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import valu_model  # noqa: E402

LOAD_THEN_WAIT = """\
_kernel:
; %bb.0:
	s_load_dwordx4 s[0:3], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
.LBB0_1:                                ; =>This Loop Header: Depth=1
	s_load_dword s5, s[16:17], 0x0
	s_waitcnt lgkmcnt(0)
	s_xor_b32 s5, s5, s6
	v_xor_b32_e32 v1, s5, v0
	v_mad_u64_u32 v[2:3], s[8:9], v1, s7, 0
	s_load_dword s18, s[22:23], 0x0
	s_load_dword s19, s[22:23], 0x10
	v_mul_f32_e32 v4, v2, v3
	v_exp_f32_e32 v4, v4
	s_waitcnt lgkmcnt(0)
	v_pk_fma_f32 v[6:7], v[4:5], s[18:19], v[6:7]
	s_cmp_lg_u32 s20, s21
	s_cbranch_scc0 .LBB0_3
.LBB0_2:                                ;   in Loop: Header=BB0_1 Depth=1
	s_add_i32 s20, s20, 1
	s_cmp_lg_u32 s20, s24
	s_cbranch_scc1 .LBB0_1
	s_branch .LBB0_4
.LBB0_3:
	global_store_dwordx4 v[8:9], v[4:7], off
	s_branch .LBB0_2
.LBB0_4:
	s_endpgm
""".splitlines()

WAIT_A_BODY_LATER = """\
_kernel:
; %bb.0:
	s_load_dword s5, s[16:17], 0x0
.LBB0_1:                                ; =>This Loop Header: Depth=1
	s_waitcnt vmcnt(0) lgkmcnt(0)
	s_xor_b32 s6, s5, s6
	s_load_dword s5, s[16:17], 0x0
	v_xor_b32_e32 v1, s6, v0
	v_mad_u64_u32 v[2:3], s[8:9], v1, s7, 0
	v_mul_f32_e32 v4, v2, v3
	s_waitcnt vmcnt(0)
	v_exp_f32_e32 v4, v4
	s_cmp_lg_u32 s20, s21
	s_cbranch_scc0 .LBB0_3
.LBB0_2:                                ;   in Loop: Header=BB0_1 Depth=1
	v_add_f32_e32 v6, v4, v6
	s_add_i32 s20, s20, 1
	s_cmp_lg_u32 s20, s24
	s_cbranch_scc1 .LBB0_1
	s_branch .LBB0_4
.LBB0_3:
	global_store_dwordx4 v[8:9], v[4:7], off
	s_branch .LBB0_2
.LBB0_4:
	s_endpgm
""".splitlines()


def _report(lines):
    hot, where = valu_model.walk_step_loop(lines)
    assert where["header"] == ".LBB0_1" and where["back_edge_to"] == ".LBB0_1"
    assert [ins for ins, _ in hot] == valu_model.step_loop(lines)[0]
    return hot, valu_model.scalar_load_waits(hot)


def test_a_load_that_is_waited_for_at_once():
    hot, rep = _report(LOAD_THEN_WAIT)
    assert not any("dwordx4" in text for _, text in hot)          # the kernel's prologue and the output block are not walked
    loads = rep["scalar_loads"]
    assert [rec["load"] for rec in loads] == ["s_load_dword s5, s[16:17], 0x0", "s_load_dword s18, s[22:23], 0x0",
                                              "s_load_dword s19, s[22:23], 0x10"]
    assert [rec["valu_between"] for rec in loads] == [0, 2, 2]
    assert [rec["next_turn"] for rec in loads] == [False, False, False]
    assert loads[0]["wait_at"] == loads[0]["at"] + 1
    assert rep["s_waitcnt_lgkmcnt0"] == 2 and len(rep["s_waitcnt"]) == 2


def test_a_load_whose_wait_is_a_loop_body_later():
    hot, rep = _report(WAIT_A_BODY_LATER)
    (rec,) = rep["scalar_loads"]
    assert rec["load"] == "s_load_dword s5, s[16:17], 0x0" and rec["at"] == 2
    # all five vector instructions of a turn lie between the load and the wait at the top of the next turn
    assert rec["next_turn"] is True and rec["wait_at"] == 0 and rec["valu_between"] == 5
    # `s_waitcnt vmcnt(0)` covers no scalar load
    assert rep["s_waitcnt_lgkmcnt0"] == 1 and [w["at"] for w in rep["s_waitcnt"]] == [0, 6]


def test_a_path_without_a_wait_reports_none():
    hot = [("s_load_dword", "s_load_dword s5, s[16:17], 0x0"), ("v_mov_b32", "v_mov_b32_e32 v0, s5")]
    (rec,) = valu_model.scalar_load_waits(hot)["scalar_loads"]
    assert rec["wait_at"] is None and rec["valu_between"] is None
