"""The soft-dice kernels keep their per-class accumulators and logits in
registers indexed by compile-time constants only: none may carry a private
segment (a spill, or a per-lane array that went to memory through a runtime
index). Read from the compiler's resource remarks via
tools/kernel_resources.py (CPU, needs hipcc)."""
import os
import shutil
import sys

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_REPO, 'coinstac_dinunet_amd', 'ops', 'csrc',
                    'segdice.hip')

_KERNELS = ('seg_sdice_reg_fwd_kernel', 'seg_sdice_reg_bwd_kernel',
            'seg_sdice_tile_fwd_kernel', 'seg_sdice_tile_bwd_kernel',
            'seg_sdice_finish_kernel')


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not found')
def test_segdice_kernels_have_no_private_segment():
    sys.path.insert(0, os.path.join(_REPO, 'tools'))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report([_SRC])
    names = ' '.join(k['name'] for k in rows)
    for kern in _KERNELS:
        assert kern in names, f'{kern} missing from the resource report'
    # each path has a 16-byte and a scalar instance, the register path at
    # both class caps
    for inst in ('seg_sdice_reg_fwd_kernel<c10::BFloat16, long, 8, 4>',
                 'seg_sdice_reg_fwd_kernel<c10::BFloat16, long, 1, 8>',
                 'seg_sdice_reg_bwd_kernel<float, unsigned char, 4, 8>',
                 'seg_sdice_reg_bwd_kernel<c10::Half, unsigned char, 1, 4>',
                 'seg_sdice_tile_fwd_kernel<c10::BFloat16, unsigned char, 8>',
                 'seg_sdice_tile_fwd_kernel<float, long, 1>',
                 'seg_sdice_tile_bwd_kernel<c10::BFloat16, long, 8>',
                 'seg_sdice_tile_bwd_kernel<c10::Half, long, 1>'):
        assert inst in names, f'{inst} missing from the resource report'
    bad = [kernel_resources.format_row(k) for k in rows
           if k.get('private') != 0]
    assert not bad, 'segdice kernels with a private segment:\n' + '\n'.join(bad)
