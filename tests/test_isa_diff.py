"""CPU: the normaliser and the pairing of tools/isa_diff.py (did a refactor change code generation?) on small synthetic
assembly texts: the same code under other local label numbers is equal, one changed operand or one changed descriptor
field is not, and a kernel that is missing on a side or defined by two units is reported."""

import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def kernel(name, index, operand="v2", vgprs=12):
    """One kernel as LLVM prints it, the `index`-th function of its translation unit."""
    return f"""
	.section	.text.{name},"axG",@progbits,{name},comdat
	.globl	{name} ; -- Begin function {name}
	.p2align	8
	.type	{name},@function
{name}: ; @{name}
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0
.LBB{index}_1:                                ; =>This Loop Header: Depth=1
	v_add_f64 v[0:1], v[0:1], {operand}   ; a comment
	s_cbranch_scc1 .LBB{index}_1
.Ltmp{index}:
; %bb.2:
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {name}
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr {vgprs}
	.end_amdhsa_kernel
	.section	.text.{name},"axG",@progbits,{name},comdat
.Lfunc_end{index}:
	.size	{name}, .Lfunc_end{index}-{name}
                                        ; -- End function
	.set {name}.num_vgpr, {vgprs}
"""


A, B = "_ZN12_GLOBAL__N_13k_aEPf", "_ZN12_GLOBAL__N_13k_bEPf"


def test_normalise_renames_the_function_index_only():
    assert isa_diff.normalise("\ts_cbranch_scc1 .LBB31_35   ; loop") == "s_cbranch_scc1 .LBB#_35"
    assert isa_diff.normalise(".Lfunc_end7:") == ".Lfunc_end#:"
    assert isa_diff.normalise("\t.long .LJTI4_0-.Ltmp12") == ".long .LJTI#_0-.Ltmp#"
    assert isa_diff.normalise("; %bb.0:") == ""


def test_kernels_takes_body_and_descriptor():
    k = isa_diff.kernels(kernel(A, 3) + kernel(B, 4))
    assert set(k) == {A, B}
    assert "v_add_f64 v[0:1], v[0:1], v2" in k[A]["insts"] and ".LBB#_1:" in k[A]["insts"]
    assert k[A]["desc"] == [".amdhsa_group_segment_fixed_size 0", ".amdhsa_next_free_vgpr 12"]
    assert not any("amdhsa" in line for line in k[A]["insts"])


def test_moved_kernel_with_other_label_numbers_is_equal():
    rows, ok = isa_diff.pair({"one.hip": kernel(A, 0) + kernel(B, 1)}, {"a.hip": kernel(A, 0), "b.hip": kernel(B, 0)})
    assert ok
    assert rows == [(A, "one.hip", "a.hip", "same", "same"), (B, "one.hip", "b.hip", "same", "same")]


def test_one_changed_operand_is_different():
    rows, ok = isa_diff.pair({"one.hip": kernel(A, 0) + kernel(B, 1)},
                             {"a.hip": kernel(A, 0), "b.hip": kernel(B, 0, operand="v3")})
    assert not ok
    assert rows == [(A, "one.hip", "a.hip", "same", "same"), (B, "one.hip", "b.hip", "DIFFERENT", "same")]


def test_one_changed_descriptor_field_is_different():
    rows, ok = isa_diff.pair({"one.hip": kernel(A, 0)}, {"a.hip": kernel(A, 0, vgprs=13)})
    assert not ok and rows == [(A, "one.hip", "a.hip", "same", "DIFFERENT")]


def test_missing_kernel_is_reported_on_either_side():
    rows, ok = isa_diff.pair({"one.hip": kernel(A, 0) + kernel(B, 1)}, {"a.hip": kernel(A, 0)})
    assert not ok and rows[1] == (B, "one.hip", "-", "missing", "missing")
    rows, ok = isa_diff.pair({"one.hip": kernel(A, 0)}, {"a.hip": kernel(A, 0), "b.hip": kernel(B, 0)})
    assert not ok and rows[1] == (B, "-", "b.hip", "missing", "missing")


def test_kernel_defined_by_two_units_is_reported():
    rows, ok = isa_diff.pair({"one.hip": kernel(A, 0)}, {"a.hip": kernel(A, 0), "b.hip": kernel(A, 0)})
    assert not ok and rows == [(A, "one.hip", "a.hip+b.hip", "duplicate", "duplicate")]
