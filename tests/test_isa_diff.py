"""tools/isa_diff.py on small canned listings: splitting, label renumbering, descriptor comparison, error messages.  No compiler."""
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "isa_diff", os.path.join(os.path.dirname(__file__), "..", "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def listing(sym, f, body, vgpr=12, tmp=5):
    return f"""
	.globl	{sym}
{sym}:                                  ; @{sym}
; %bb.0:
	s_load_dword s4, s[0:1], 0x0           ; a comment
	s_cbranch_scc1 .LBB{f}_2
.Ltmp{tmp}:
{body}
.LBB{f}_2:
	s_endpgm
.Lfunc_end{f}:
	.size	{sym}, .Lfunc_end{f}-{sym}
	.section	.rodata
	.amdhsa_kernel {sym}
		.amdhsa_next_free_vgpr {vgpr}
		.amdhsa_group_segment_fixed_size 0
	.end_amdhsa_kernel
"""


def test_same_kernel_at_another_function_index_is_identical():
    a = isa_diff.split_kernels(listing("_Z1kv", 3, "\tv_mov_b32_e32 v0, 0"))
    b = isa_diff.split_kernels(listing("_Z1kv", 12, "\tv_mov_b32_e32 v0, 0", tmp=9))
    assert a == b
    text, desc = a["_Z1kv"]
    assert ".amdhsa_next_free_vgpr 12" in desc and all(";" not in t for t in text)


def test_instruction_and_descriptor_differences_are_seen():
    base = isa_diff.split_kernels(listing("_Z1kv", 3, "\tv_mov_b32_e32 v0, 0"))["_Z1kv"]
    text = isa_diff.split_kernels(listing("_Z1kv", 3, "\tv_mov_b32_e32 v0, 1"))["_Z1kv"]
    desc = isa_diff.split_kernels(listing("_Z1kv", 3, "\tv_mov_b32_e32 v0, 0", vgpr=13))["_Z1kv"]
    assert text[0] != base[0] and text[1] == base[1]
    assert desc[0] == base[0] and desc[1] != base[1]


def test_distinct_labels_stay_distinct():
    one = "\ts_branch .Ltmp5\n.Ltmp7:"
    two = "\ts_branch .Ltmp7\n.Ltmp7:"
    a = isa_diff.split_kernels(listing("_Z1kv", 3, one))["_Z1kv"][0]
    b = isa_diff.split_kernels(listing("_Z1kv", 3, two))["_Z1kv"][0]
    assert a != b


def test_two_kernels_are_split():
    both = listing("_Z1av", 0, "\tv_mov_b32_e32 v0, 0") + listing("_Z1bv", 1, "\tv_mov_b32_e32 v0, 0")
    ks = isa_diff.split_kernels(both)
    assert sorted(ks) == ["_Z1av", "_Z1bv"] and ks["_Z1av"] == ks["_Z1bv"]


def test_broken_listings_name_the_symbol():
    good = listing("_Z1kv", 3, "\tv_mov_b32_e32 v0, 0")
    with pytest.raises(RuntimeError, match="_Z1kv"):
        isa_diff.split_kernels(good[:good.index("\t.end_amdhsa_kernel")])
    with pytest.raises(RuntimeError, match="_Z1kv.*no body"):
        isa_diff.split_kernels(good[good.index("\t.section"):])
    with pytest.raises(RuntimeError, match="_Z1kv.*\\.size"):
        isa_diff.split_kernels(good.replace("\t.size\t_Z1kv", "\t.type\t_Z1kv"))


def test_rename_without_a_demangler_fails(monkeypatch):
    monkeypatch.setattr(isa_diff.shutil, "which", lambda name: None)
    assert isa_diff.demangle(["_Z1kv"]) == {"_Z1kv": "_Z1kv"}
    with pytest.raises(RuntimeError, match="demangled"):
        isa_diff.demangle(["_Z1kv"], need=True)
