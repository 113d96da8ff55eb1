"""tools/kernel_isa_diff.py: the splitter, the normaliser and the comparison on three short hand-written assembly texts (no compiler)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import kernel_isa_diff as K  # noqa: E402


def _kernel(name, index, label0, body, lds=0):
    """One kernel the way the AMDGPU backend prints it: function `index` of its file (the <function> of .LBB<function>_<n> and of
    .Lfunc_end<function>), its basic blocks numbered from `label0`."""
    return """
	.protected	{n}
	.globl	{n}
	.p2align	8
	.type	{n},@function
{n}:                                    ; @{n}
; %bb.0:
	s_load_dwordx2 s[2:3], s[0:1], 0x0
	v_cmp_gt_i32_e32 vcc, 4, v0             ; a comment
	s_cbranch_vccz .LBB{i}_{l1}
; %bb.1:
{body}
.LBB{i}_{l1}:
	s_cbranch_execz .LBB{i}_{l2}

.LBB{i}_{l2}:                               ; %exit
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {n}
		.amdhsa_group_segment_fixed_size {lds}
		.amdhsa_next_free_vgpr 8
	.end_amdhsa_kernel
	.text
.Lfunc_end{i}:
	.size	{n}, .Lfunc_end{i}-{n}
                                        ; -- End function
	.set {n}.num_vgpr, 8
""".format(n=name, i=index, l1=label0, l2=label0 + 1, body=body, lds=lds)


HEAD = '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n\t.text\n'
A, B = "_ZN3dyt8a_kernelEPfi", "_ZN3dyt8b_kernelIfEEvPT_"
BODY_A = "\tv_add_f32_e32 v1, v1, v2\n\tglobal_store_dword v0, v1, s[2:3]"
BODY_B = "\tv_mul_f32_e32 v1, v1, v2\n\tglobal_store_dword v0, v1, s[2:3]"

ORIGINAL = HEAD + _kernel(A, 0, 1, BODY_A) + _kernel(B, 1, 1, BODY_B, lds=1024)
REORDERED = HEAD + _kernel(B, 0, 1, BODY_B, lds=1024) + _kernel(A, 7, 1, BODY_A)   # other order, other function indices in the labels
CHANGED = HEAD + _kernel(A, 0, 1, BODY_A) + _kernel(B, 1, 1, BODY_B.replace("v_mul_f32", "v_fma_f32"), lds=2048)


def _pool(text):
    return {name: [unit] for name, (unit, _) in K.split_units(text).items()}


def test_split_finds_both_kernels_with_their_descriptors():
    units = K.split_units(ORIGINAL)
    assert sorted(units) == sorted([A, B])
    for name, (unit, is_kernel) in units.items():
        assert is_kernel
        assert unit.startswith(name + ":") and unit.endswith(".Lfunc_end:")
        assert ".amdhsa_kernel " + name in unit and ".end_amdhsa_kernel" in unit
        assert ";" not in unit and "\n\n" not in unit
    assert ".amdhsa_group_segment_fixed_size 1024" in units[B][0] and "1024" not in units[A][0]
    assert "s_cbranch_vccz .LBB_1" in units[A][0] and ".LBB_2:" in units[A][0]


def test_order_and_label_indices_do_not_matter():
    assert K.compare(_pool(ORIGINAL), _pool(REORDERED)) == ([], [], [])
    # the labels still count inside a function: two branches to one label are not two branches to two
    merged = ORIGINAL.replace("s_cbranch_execz .LBB0_2", "s_cbranch_execz .LBB0_1")
    assert K.compare(_pool(ORIGINAL), _pool(merged)) == ([], [], [A])


def test_a_changed_instruction_and_descriptor_value_name_that_kernel():
    assert K.compare(_pool(ORIGINAL), _pool(CHANGED)) == ([], [], [B])
    only_descriptor = ORIGINAL.replace(".amdhsa_group_segment_fixed_size 1024", ".amdhsa_group_segment_fixed_size 2048")
    assert K.compare(_pool(ORIGINAL), _pool(only_descriptor)) == ([], [], [B])


def test_missing_and_added_kernels_are_named():
    only_a = HEAD + _kernel(A, 0, 1, BODY_A)
    assert K.compare(_pool(ORIGINAL), _pool(only_a)) == ([B], [], [])
    assert K.compare(_pool(only_a), _pool(ORIGINAL)) == ([], [B], [])
