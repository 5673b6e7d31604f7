"""The memory-counter model and the wait-state check of tools/asmemu.py on hand-written snippets: for every rule one snippet that is
accepted and its twin - the wait removed, or its count off by one - that is rejected BY THAT RULE (the error text is matched)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asmemu  # noqa: E402

QP = "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
IN_FLIGHT = r"touches v%d, the destination of `%s.*still in flight"
DATA_SOURCE = r"loads into v%d, the data source of `%s.*still in its queue"
AT_END = r"the block ends with `%s.*still in flight"
BY_DPP = r"reads v%d by DPP %d wait state\(s\) behind the VALU write of it: 2 are required"
SADDR = r"takes its address from s%d %d wait state\(s\) behind the VALU write of it: 5 are required"
STORE_DATA = r"overwrites v%d %d wait state\(s\) behind `global_store_dwordx4.*which stores it: 2 are required"


def run(text, lanes=4, **kw):
    """the snippet on four lanes: s[0:1] = a global buffer of 4 KiB, v1 = 16 x lane, v[10:13] = data; LDS holds 4 KiB of words"""
    emu = asmemu.Emu(lanes=lanes, **kw)
    emu.s[0], emu.s[1] = 0x10000, 0
    emu.v[1] = [16 * lane for lane in range(lanes)]
    for k in range(4):
        emu.v[10 + k] = [100 * k + lane for lane in range(lanes)]
    for a in range(0, 4096, 4):
        emu.mem[0x10000 + a] = a
        emu.lds[a] = a + 1
    emu.run([l for l in text.split("\n") if l.strip()])
    return emu


def rejected(text, pattern, **kw):
    with pytest.raises(RuntimeError, match=pattern):
        run(text, **kw)


# ------------------------------------------------------------------------------------------------------------ (a) loads in flight
def test_a_global_load_is_waited_for_before_its_destination_is_read():
    text = """
        global_load_dwordx2 v[2:3], v1, s[0:1]
        v_mov_b32 v4, 7
        %s
        v_add_u32 v5, v2, v4
    """
    emu = run(text % "s_waitcnt vmcnt(0)")
    assert emu.v[5] == [16 * lane + 7 for lane in range(4)] and not emu.vmq
    rejected(text % "", IN_FLIGHT % (2, "global_load_dwordx2"))
    # a wait for the other counter leaves the VM queue alone
    rejected(text % "s_waitcnt lgkmcnt(0)", IN_FLIGHT % (2, "global_load_dwordx2"))


def test_vmcnt_retires_in_order_all_but_the_youngest():
    text = """
        global_load_dwordx2 v[2:3], v1, s[0:1]
        global_load_dwordx2 v[4:5], v1, s[0:1] offset:8
        s_waitcnt vmcnt(%d)
        v_add_u32 v6, v2, v3
        s_waitcnt vmcnt(0)
        v_add_u32 v7, v4, v5
    """
    emu = run(text % 1)
    assert emu.v[6] == [32 * lane + 4 for lane in range(4)] and emu.v[7] == [32 * lane + 20 for lane in range(4)]
    rejected(text % 2, IN_FLIGHT % (2, "global_load_dwordx2 v\\[2:3\\]"))
    # the younger load is the one vmcnt(1) leaves in flight
    rejected(text.replace("v_add_u32 v6, v2, v3", "v_add_u32 v6, v4, v3") % 1, IN_FLIGHT % (4, "global_load_dwordx2 v\\[4:5\\]"))


def test_an_lds_read_is_waited_for_before_its_destination_is_read_or_overwritten():
    text = """
        ds_read_b64 v[2:3], v1
        ds_read_b64 v[4:5], v1 offset:8
        v_mov_b32 v6, 1
        s_waitcnt lgkmcnt(%d)
        %s
        s_waitcnt lgkmcnt(0)
        v_add_u32 v7, v4, v2
    """
    emu = run(text % (1, "v_add_u32 v6, v2, v6"))
    assert emu.v[7] == [32 * lane + 1 + 9 for lane in range(4)]
    rejected(text % (2, "v_add_u32 v6, v2, v6"), IN_FLIGHT % (2, "ds_read_b64 v\\[2:3\\]"))
    run(text % (1, "v_mov_b32 v3, 0"))
    rejected(text % (2, "v_mov_b32 v3, 0"), IN_FLIGHT % (3, "ds_read_b64 v\\[2:3\\]"))          # an overwrite: the load would land on top of it
    rejected(text % (1, "ds_read_b64 v[4:5], v1 offset:16"), IN_FLIGHT % (4, "ds_read_b64 v\\[4:5\\]"))


def test_a_count_that_cannot_be_encoded_is_an_error():
    text = """
        ds_read_b64 v[2:3], v1
        s_waitcnt %s
        s_waitcnt vmcnt(0) lgkmcnt(0)
    """
    run(text % "vmcnt(63) lgkmcnt(15)")
    rejected(text % "vmcnt(64)", r"vmcnt\(64\) cannot be encoded \(at most 63\)")
    rejected(text % "lgkmcnt(16)", r"lgkmcnt\(16\) cannot be encoded \(at most 15\)")


def test_a_scalar_load_makes_every_nonzero_lgkmcnt_worthless():
    text = """
        ds_read_b64 v[2:3], v1
        %s
        s_waitcnt lgkmcnt(%d)
        v_add_u32 v4, v2, v3
        s_waitcnt lgkmcnt(0)
    """
    run(text % ("ds_read_b64 v[6:7], v1 offset:8", 1))                 # in order: one left in flight is the younger one
    rejected(text % ("s_load_dwordx2 s[4:5], s[0:1], 0x0", 1), IN_FLIGHT % (2, "ds_read_b64"))
    emu = run(text % ("s_load_dwordx2 s[4:5], s[0:1], 0x0", 0))
    assert (emu.s[4], emu.s[5]) == (0, 4) and emu.smem_seen


# ----------------------------------------------------------------------------------------------- (b) stores that still hold their data
def test_a_load_may_not_land_in_the_data_registers_of_a_queued_lds_write():
    """the idiom of k_miller1: two landing writes, reads behind them, then a count that lets exactly the two writes through"""
    text = """
        ds_write_b64 v1, v[10:11]
        ds_write_b64 v1, v[12:13] offset:8
        ds_read_b64 v[2:3], v1 offset:2048
        s_waitcnt lgkmcnt(%d)
        global_load_dwordx2 v[12:13], v1, s[0:1]
        s_waitcnt vmcnt(0) lgkmcnt(0)
        v_add_u32 v4, v12, v2
    """
    emu = run(text % 1)
    assert emu.v[4] == [16 * lane + 16 * lane + 2049 for lane in range(4)] and emu.lds[8] == 200
    rejected(text % 2, DATA_SOURCE % (12, "ds_write_b64 v1, v\\[12:13\\]"))
    rejected(text.replace("s_waitcnt lgkmcnt(%d)", "") % (), DATA_SOURCE % (12, "ds_write_b64"))


def test_a_load_may_not_land_in_the_data_registers_of_a_queued_global_store():
    text = """
        global_store_dwordx4 v1, v[10:13], s[0:1]
        v_mov_b32 v4, 0
        %s
        ds_read_b64 v[10:11], v1
        s_waitcnt lgkmcnt(0)
    """
    emu = run(text % "s_waitcnt vmcnt(0)")
    assert emu.mem[0x10000 + 16 + 4] == 101 and emu.v[10] == [16 * lane + 1 for lane in range(4)]
    rejected(text % "", DATA_SOURCE % (10, "global_store_dwordx4"))


# ------------------------------------------------------------------------------------------------------------ (c) the end of the text
def test_nothing_is_in_flight_where_the_block_ends():
    text = """
        v_mov_b32 v4, 0
        ds_write_b64 v1, v[10:11]
        global_load_dwordx2 v[2:3], v1, s[0:1]
        ds_read_b64 v[6:7], v1 offset:1024
        %s
    """
    run(text % "s_waitcnt vmcnt(0) lgkmcnt(0)")
    rejected(text % "s_waitcnt vmcnt(0)", AT_END % "ds_read_b64")
    rejected(text % "s_waitcnt lgkmcnt(0)", AT_END % "global_load_dwordx2")
    rejected(text % "s_waitcnt vmcnt(0) lgkmcnt(1)", AT_END % "ds_read_b64")
    # a store may still be on its way (it needs no register any more): only loads are held to this
    run("""
        ds_write_b64 v1, v[10:11]
        global_store_dwordx4 v1, v[10:13], s[0:1]
        s_nop 1
    """)


def test_the_queues_follow_the_path_that_is_executed():
    text = """
        ds_read_b64 v[2:3], v1
        s_cmp_eq_u32 s0, %s
        s_cbranch_scc1 .Lskip
        s_waitcnt lgkmcnt(0)
        .Lskip:
        v_add_u32 v4, v2, v3
        s_waitcnt lgkmcnt(0)
    """
    run(text % "0")                                                     # not taken: the wait is on the path
    rejected(text % "0x10000", IN_FLIGHT % (2, "ds_read_b64"))      # taken: it is not


# ------------------------------------------------------------------------------------------------------------ wait states
def test_dpp_reads_a_vgpr_two_states_behind_its_valu_write():
    text = """
        v_mov_b32 v2, v1
        %s
        v_mov_b32_dpp v3, v2 """ + QP + """
        v_add_u32_dpp v4, v3, v2 """ + QP + """
    """
    with pytest.raises(RuntimeError, match=BY_DPP % (3, 0)):           # (the second DPP instruction reads what the first one wrote)
        run(text % "s_nop 1")
    text = text.replace("v_add_u32_dpp v4, v3, v2", "v_add_u32_dpp v4, v1, v2")
    emu = run(text % "s_nop 1")
    assert emu.v[3] == [16, 0, 48, 32] and emu.v[4] == [16 + 0, 0 + 16, 48 + 32, 32 + 48]
    rejected(text % "s_nop 0", BY_DPP % (2, 1))
    rejected(text % "", BY_DPP % (2, 0))
    run(text % "v_mov_b32 v5, 0\nv_mov_b32 v6, 0")                      # any two instructions are two states
    rejected(text % "v_mov_b32 v5, 0", BY_DPP % (2, 1))
    run(text % "", wait_states=False)


def test_vector_memory_takes_a_valu_written_address_register_five_states_later():
    text = """
        v_readfirstlane_b32 s4, v20
        s_mov_b32 s5, 0
        %s
        global_load_dwordx2 v[2:3], v1, s[4:5]
        s_waitcnt vmcnt(0)
    """

    def go(pad, **kw):
        emu = asmemu.Emu(lanes=4, **kw)
        emu.v[1], emu.v[20] = [16 * lane for lane in range(4)], [0x10000] * 4
        for a in range(0, 64, 4):
            emu.mem[0x10000 + a] = a
        return emu.run([l for l in (text % pad).split("\n") if l.strip()])

    assert go("s_nop 3").v[3] == [16 * lane + 4 for lane in range(4)]
    with pytest.raises(RuntimeError, match=SADDR % (4, 4)):
        go("s_nop 2")
    with pytest.raises(RuntimeError, match=SADDR % (4, 1)):
        go("")
    go("", wait_states=False)
    # the scalar unit's own writes are interlocked: the table pointer of k_coop's MULACC block is advanced right in front of its load
    run("""
        s_add_u32 s0, s0, 16
        s_addc_u32 s1, s1, 0
        global_load_dwordx2 v[2:3], v1, s[0:1]
        s_waitcnt vmcnt(0)
    """)


def test_the_data_registers_of_a_wide_store_are_rewritten_two_states_later():
    text = """
        global_store_dwordx4 v1, v[10:13], s[0:1]
        %s
        v_mov_b32 v12, 0
        s_waitcnt vmcnt(0)
    """
    emu = run(text % "s_nop 1")
    assert emu.mem[0x10000 + 8] == 200 and emu.v[12] == [0] * 4
    rejected(text % "s_nop 0", STORE_DATA % (12, 1))
    rejected(text % "", STORE_DATA % (12, 0))
    run(text % "s_waitcnt vmcnt(0)")                                    # the store is through: nothing to wait for
