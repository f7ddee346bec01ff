"""Every spatial conv3d instance keeps its working set in registers (no
private segment) and its LDS at or below 81,920 B, so two workgroups share
a CU. Read from the compiler's own resource remarks via
tools/kernel_resources.py (CPU only, needs hipcc)."""
import os
import shutil
import sys

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_REPO, 'coinstac_dinunet_amd', 'ops', 'csrc')
_KERNELS = ('conv3d_spatial_kernel', 'conv3d_dgrad_s2_sp_kernel')


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not found')
def test_spatial_kernels_fit_registers_and_two_per_cu():
    sys.path.insert(0, os.path.join(_REPO, 'tools'))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report(
        [os.path.join(_CSRC, 'conv3d_spatial.hip')])
    rows = [k for k in rows
            if any(n in k['name'] or n in k['mangled'] for n in _KERNELS)]
    names = ' '.join(k['name'] + ' ' + k['mangled'] for k in rows)
    for kern in _KERNELS:
        assert kern in names, f'{kern} missing from the resource report'
    bad = [kernel_resources.format_row(k) for k in rows
           if k.get('private') != 0 or not 0 <= k.get('lds', -1) <= 81920]
    assert not bad, ('spatial kernels with a private segment or more than '
                     '81,920 B of LDS:\n' + '\n'.join(bad))
