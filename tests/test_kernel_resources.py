"""No wgrad kernel may carry a private segment: its accumulators live in
registers, and a runtime index into the array (or a spill) would move them
to memory on every chunk-loop iteration. Read from the compiler's own
resource remarks via tools/kernel_resources.py (CPU only, needs hipcc)."""
import os
import shutil
import sys

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_REPO, 'coinstac_dinunet_amd', 'ops', 'csrc')


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not found')
def test_wgrad_kernels_have_no_private_segment():
    sys.path.insert(0, os.path.join(_REPO, 'tools'))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report(
        [os.path.join(_CSRC, 'conv3d.hip'), os.path.join(_CSRC, 'conv2d.hip')],
        name_filter='wgrad')
    names = ' '.join(k['name'] for k in rows)
    for kern in ('conv3d_wgrad_s1_kernel', 'conv3d_wgrad_s1_db_kernel',
                 'conv2d_wgrad_sp_kernel'):
        assert kern in names, f'{kern} missing from the resource report'
    bad = [kernel_resources.format_row(k) for k in rows
           if k.get('private') != 0]
    assert not bad, 'wgrad kernels with a private segment:\n' + '\n'.join(bad)
