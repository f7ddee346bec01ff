"""The segmentation-head kernels are streaming kernels with a handful of
live values per lane: none may carry a private segment (a spill, or a
per-lane vector that went to memory through a runtime index). Read from the
compiler's resource remarks via tools/kernel_resources.py (CPU, needs
hipcc)."""
import os
import shutil
import sys

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_REPO, 'coinstac_dinunet_amd', 'ops', 'csrc',
                    'segloss.hip')

_KERNELS = ('seg_dice_fwd_kernel', 'seg_dice_finish_kernel',
            'seg_dice_bwd_kernel', 'seg_ce_fwd_kernel',
            'seg_ce_finish_kernel', 'seg_ce_bwd_kernel',
            'seg_prf1a_kernel', 'seg_confusion_kernel')


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not found')
def test_segloss_kernels_have_no_private_segment():
    sys.path.insert(0, os.path.join(_REPO, 'tools'))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report([_SRC])
    names = ' '.join(k['name'] for k in rows)
    for kern in _KERNELS:
        assert kern in names, f'{kern} missing from the resource report'
    # every logits dtype has a 16-byte and a scalar instance
    for inst in ('seg_ce_fwd_kernel<c10::BFloat16, long, 8>',
                 'seg_ce_fwd_kernel<c10::BFloat16, long, 1>',
                 'seg_dice_bwd_kernel<float, unsigned char, false, 4>'):
        assert inst in names, f'{inst} missing from the resource report'
    bad = [kernel_resources.format_row(k) for k in rows
           if k.get('private') != 0]
    assert not bad, 'segloss kernels with a private segment:\n' + '\n'.join(bad)
