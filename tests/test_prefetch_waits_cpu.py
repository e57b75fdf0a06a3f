"""scripts/prefetch_waits.py on a few hand-written lines of gfx9 assembly: a kernel with one stage loop that prefetches four loads per trip,
once with the wait where it belongs (the hand-over at the top of the next trip) and once with an early wait right behind the issue."""
import io
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import prefetch_waits as PW  # noqa: E402

OTHER = """
_Z7k_otherILi2ELi0EEvPd:                ; @_Z7k_otherILi2ELi0EEvPd
	s_waitcnt vmcnt(0)
	s_endpgm
.Lfunc_end0:
"""

HEAD = """
	.globl	_Z6k_demoILi2ELi0ELb0EEvPd
_Z6k_demoILi2ELi0ELb0EEvPd:             ; @_Z6k_demoILi2ELi0ELb0EEvPd
; %bb.0:
	s_load_dwordx4 s[0:3], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
	global_load_dwordx2 v[2:3], v0, s[0:1]
	global_load_dwordx2 v[4:5], v0, s[0:1] offset:8
	global_load_dwordx2 v[6:7], v0, s[0:1] offset:16
	global_load_dwordx4 v[8:11], v0, s[0:1] offset:32
.LBB1_1:                                ; =>This Inner Loop Header: Depth=1
	s_waitcnt vmcnt(3)
	ds_write_b64 v1, v[2:3]
	s_waitcnt vmcnt(1)
	ds_write2_b64 v1, v[4:5], v[6:7] offset0:1 offset1:2
	s_waitcnt vmcnt(0)
	ds_write2_b64 v1, v[8:9], v[10:11] offset0:3 offset1:4
	s_add_u32 s0, s0, 64
	global_load_dwordx2 v[2:3], v0, s[0:1]
	global_load_dwordx2 v[4:5], v0, s[0:1] offset:8
	v_mov_b32_e32 v20, 0
	global_load_dwordx2 v[6:7], v0, s[0:1] offset:16
	global_load_dwordx4 v[8:11], v0, s[0:1] offset:32
"""

EARLY = """	s_waitcnt vmcnt(2)
	v_add_f64 v[12:13], v[2:3], v[4:5]
"""

TAIL = """	v_fma_f64 v[14:15], v[12:13], v[12:13], v[14:15]
	v_fma_f64 v[14:15], v[12:13], v[12:13], v[14:15]
	v_mfma_f64_16x16x4_f64 v[30:37], v[14:15], v[14:15], v[30:37]
	v_cmp_gt_u32_e32 vcc, 17, v0
	s_and_saveexec_b64 s[8:9], vcc
	s_cbranch_execz .LBB1_3
; %bb.2:                                ;   in Loop: Header=BB1_1 Depth=1
	global_store_dwordx2 v0, v[14:15], s[2:3]
.LBB1_3:                                ;   in Loop: Header=BB1_1 Depth=1
	s_or_b64 exec, exec, s[8:9]
	s_add_i32 s6, s6, 1
	s_cmp_lt_i32 s6, s7
	s_cbranch_scc1 .LBB1_1
; %bb.4:
	s_endpgm
.Lfunc_end1:
	.size	_Z6k_demoILi2ELi0ELb0EEvPd, .Lfunc_end1-_Z6k_demoILi2ELi0ELb0EEvPd
"""


def _kernel(early):
    text = OTHER + HEAD + (EARLY if early else "") + TAIL
    sym, ins, labels = PW.parse_kernel(text.split("\n"), "k_demo<2,0,false>")
    cfg = PW.Cfg(ins, labels)
    return sym, ins, labels, cfg, PW.find_loops(cfg)


def test_names_and_wait_counts():
    assert PW.mangled_fragment("k_qp_solve<17,4,false>") == "10k_qp_solveILi17ELi4ELb0EE"
    assert PW.mangled_fragment("slsqp::k_sweep<4, 1, true>") == "7k_sweepILi4ELi1ELb1EE"
    assert PW.mangled_fragment("_Z3foov") == "_Z3foov"
    assert PW.vmcnt_of("vmcnt(7) lgkmcnt(0)") == 7
    assert PW.vmcnt_of("lgkmcnt(0)") is None
    assert PW.vmcnt_of("0") == 0 and PW.vmcnt_of("0xc07f") is None      # every field 0; vmcnt = 63 (no wait), lgkmcnt(0)
    assert PW.landed(4, 0, 0) == 4 and PW.landed(4, 3, 0) == 1 and PW.landed(4, 3, 1) == 2 and PW.landed(4, 9, 1) == 0


def test_parser_finds_the_kernel_its_loop_and_the_load_group():
    sym, ins, labels, cfg, loops = _kernel(early=False)
    assert sym == "_Z6k_demoILi2ELi0ELb0EEvPd"
    assert ins[0].op == "s_load_dwordx4" and ins[-1].op == "s_endpgm"          # the other kernel's lines are not part of it
    assert set(labels) == {".LBB1_1", ".LBB1_3"}
    assert len(loops) == 1 and loops[0].head == labels[".LBB1_1"]
    in_loop = [ins[i].op for i in PW.loop_instructions(cfg, loops[0])]
    assert in_loop[0] == "s_waitcnt" and in_loop[-1] == "s_cbranch_scc1" and "s_endpgm" not in in_loop
    groups = PW.load_groups(cfg, loops, loops[0], gap=16)
    assert len(groups) == 1 and len(groups[0].members) == 4                    # the prologue's loads lie outside the loop; the v_mov does not split the run
    assert [ins[i].args.split(",")[0] for i in groups[0].members] == ["v[2:3]", "v[4:5]", "v[6:7]", "v[8:11]"]
    assert PW.load_groups(cfg, loops, loops[0], gap=1)[0].members == groups[0].members[:2]
    # the store sits under `if (lane < 17)`: the walk takes the block as entered
    b = cfg.block_of[labels[".LBB1_3"] - 1]
    assert ins[cfg.end[b]].op == "global_store_dwordx2" and cfg.live_succ[cfg.block_of[groups[0].last]] == [b]


def test_late_wait_lands_the_prefetch_in_the_hand_over():
    _, ins, labels, cfg, loops = _kernel(early=False)
    (g, trip, rows), = PW.analyse_loop(cfg, loops, loops[0])
    # from the last load: 3 x work, v_cmp, saveexec, execz, store, s_or, add, cmp, branch = 11, then the waits at the top
    assert [(ins[h.idx].args, h.dist, some, every) for h, some, every in rows] == [("vmcnt(3)", 12, 2, 2), ("vmcnt(1)", 14, 2, 2)]
    assert all(h.pmin == h.pmax == 1 for h, _, _ in rows)                      # the store was issued behind the group, so vmcnt(1) already lands all four
    assert trip == 12 + 6 + 5                                                  # ... to the top, 6 hand-over instructions and the s_add, the group itself
    out = io.StringIO()
    total = PW.report(cfg, labels, loops, {".LBB1_1": "stage loop"}, 16, 4, out=out)
    assert total == {".LBB1_1": (0, 4)}
    text = out.getvalue()
    assert "loop .LBB1_1 [stage loop]" in text and "1 mfma, 4 vector loads (0 scratch), 1 vector stores" in text
    assert "landed in the first 40 % of the trip that issued them: 0 of 4" in text


def test_early_wait_lands_it_in_the_stage_that_issued_it():
    _, ins, labels, cfg, loops = _kernel(early=True)
    (g, trip, rows), = PW.analyse_loop(cfg, loops, loops[0])
    h, some, every = rows[0]
    assert (ins[h.idx].args, h.dist, some, every, h.pmin, h.pmax) == ("vmcnt(2)", 1, 2, 2, 0, 0)       # placed for v[2:3] and v[4:5]: lands just these
    # at the top vmcnt(3) lands 4 + 1 - 3 = 2 loads, the two that have landed already; the other two wait for vmcnt(1)
    assert [(ins[h.idx].args, some) for h, some, _ in rows[1:]] == [("vmcnt(1)", 2)]
    out = io.StringIO()
    assert PW.report(cfg, labels, loops, {}, 16, 4, out=out) == {".LBB1_1": (2, 4)}
    assert PW.report(cfg, labels, loops, {}, 16, 4, only_named=True, out=out) == {}
    assert PW.report(cfg, labels, loops, {}, 16, 5, out=out) == {}             # no group of five loads


NO_WAY_BACK = """
_Z6k_demoILi2ELi0ELb0EEvPd:             ; @_Z6k_demoILi2ELi0ELb0EEvPd
	s_load_dwordx4 s[0:3], s[4:5], 0x0
.LBB2_1:
	s_and_saveexec_b64 s[8:9], vcc
	s_cbranch_execnz .LBB2_3
; %bb.2:
	global_load_dwordx2 v[2:3], v0, s[0:1]
	global_load_dwordx2 v[4:5], v0, s[0:1] offset:8
	global_load_dwordx2 v[6:7], v0, s[0:1] offset:16
	global_load_dwordx2 v[8:9], v0, s[0:1] offset:24
@A@.LBB2_3:
	s_or_b64 exec, exec, s[8:9]
@B@	s_add_i32 s6, s6, 1
	s_cmp_lt_i32 s6, s7
	s_cbranch_scc1 .LBB2_1
	s_endpgm
.Lfunc_end2:
"""


def test_a_trip_that_cannot_be_found_is_not_reported_as_a_late_wait():
    """The walk takes a forward s_cbranch_execnz as taken, so from this group there is no way back to its next issue: the trip is unknown.  A
    wait right behind the issue is early all the same; one further on is reported as not placed, never as late."""
    work = "".join("\tv_fma_f64 v[14:15], v[12:13], v[12:13], v[14:15]\n" for _ in range(20))
    for wait_at, expect, words in ((0, (4, 4), "4 of 4"), (1, (0, 4), "0 of 4 (4 more landed at a place in the trip that could not be found)")):
        a, b = ("\ts_waitcnt vmcnt(0)\n", "") if wait_at == 0 else ("", work + "\ts_waitcnt vmcnt(0)\n")
        text = NO_WAY_BACK.replace("@A@", a).replace("@B@", b)
        sym, ins, labels = PW.parse_kernel(text.split("\n"), "k_demo<2,0,false>")
        cfg = PW.Cfg(ins, labels)
        loops = PW.find_loops(cfg)
        (g, trip, rows), = PW.analyse_loop(cfg, loops, loops[0])
        assert trip is None and len(rows) == 1 and rows[0][1] == 4
        out = io.StringIO()
        assert PW.report(cfg, labels, loops, {}, 16, 4, out=out) == {".LBB2_1": expect}
        assert "(  ? % of the trip)" in out.getvalue() and "issued them: " + words in out.getvalue()
