#!/usr/bin/env python3
"""Instruction counts by class, per basic block, of one kernel in a gfx950 assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only quadtree-mpnnlstm_amd/csrc/gatecell.hip -o gatecell.s
    python profiles/isa_count.py gatecell.s 'k_gate_cell_pILi2ELi4ELi8E'

Prints one line per basic block (label, instruction count, counts by class) and the kernel's total.  The unit loop of a
persistent kernel is the block(s) a backward branch returns to; straight-line kernels have their phases in label order.
"""
import collections
import re
import sys


def classify(op):
    if op.startswith('v_mfma') or op.startswith('v_smfma'):
        return 'mfma'
    if op.startswith(('v_exp', 'v_rcp', 'v_rsq', 'v_sqrt', 'v_log', 'v_sin', 'v_cos')):
        return 'trans'
    if op.startswith(('v_div_scale', 'v_div_fmas', 'v_div_fixup')):
        return 'div'
    if op.startswith(('v_lshl_add_u64', 'v_add_co', 'v_addc_co', 'v_mad_u64', 'v_mad_i64', 'v_lshlrev_b64', 'v_ashrrev_i64',
                      'v_cmp_gt_i64', 'v_cmp_lt_i64', 'v_cmp_le_i64', 'v_cmp_ge_i64', 'v_cmp_gt_u64', 'v_cmp_lt_u64')):
        return 'valu_i64'
    if op.startswith('v_cndmask') or op.startswith('v_cmp'):
        return 'valu_sel'
    if op.endswith('_dpp') or op.startswith('v_mov_b32_dpp'):
        return 'valu_dpp'
    if op.startswith('v_accvgpr'):
        return 'accmov'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('ds_bpermute') or op.startswith('ds_swizzle') or op.startswith('ds_permute'):
        return 'lds_shfl'
    if op.startswith('ds_read') or op.startswith('ds_load'):
        return 'lds_rd'
    if op.startswith('ds_write') or op.startswith('ds_store'):
        return 'lds_wr'
    if op.startswith(('global_load', 'buffer_load', 'flat_load')):
        return 'vmem_rd'
    if op.startswith(('global_store', 'buffer_store', 'flat_store')):
        return 'vmem_wr'
    if op.startswith(('scratch_load', 'scratch_store')):
        return 'scratch'
    if op.startswith('s_waitcnt'):
        return 'waitcnt'
    if op.startswith(('s_cbranch', 's_branch')):
        return 'branch'
    if op.startswith('s_load') or op.startswith('s_buffer_load'):
        return 'smem'
    if op.startswith('s_'):
        return 'salu'
    return 'other'


def main(path, pat):
    lines = open(path).read().split('\n')
    start = next(i for i, l in enumerate(lines) if re.match(r'^_Z\w*' + re.escape(pat) + r'\w*:', l))
    blocks, cur = [], ['entry', collections.Counter(), []]
    for l in lines[start + 1:]:
        if l.startswith('.Lfunc_end'):
            break
        m = re.match(r'^(\.LBB\w+):', l)
        if m:
            blocks.append(cur)
            cur = [m.group(1), collections.Counter(), []]
            continue
        m = re.match(r'^\s+([a-z][a-z0-9_]+)\b(.*)', l)
        if not m or m.group(1).startswith('.'):
            continue
        op = m.group(1)
        cur[1][classify(op)] += 1
        if op.startswith(('s_cbranch', 's_branch')):
            cur[2].append(m.group(2).split(';')[0].strip())
    blocks.append(cur)
    total = collections.Counter()
    for name, c, br in blocks:
        total.update(c)
        print(f'{name:14s} {sum(c.values()):5d}  ' + ' '.join(f'{k}={v}' for k, v in sorted(c.items())) + (f'  -> {",".join(br)}' if br else ''))
    print(f'{"TOTAL":14s} {sum(total.values()):5d}  ' + ' '.join(f'{k}={v}' for k, v in sorted(total.items())))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
