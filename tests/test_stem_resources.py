"""The first-layer kernels keep their working set in registers: the one-pass
BN-backward + wgrad kernel (both row widths), its finish kernel and the
single-channel forward instances with epilogue statistics must carry no
private segment. Read from the compiler's resource remarks via
tools/kernel_resources.py (CPU, needs hipcc)."""
import os
import shutil
import sys

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_REPO, 'coinstac_dinunet_amd', 'ops', 'csrc')

# conv3d_spatial_kernel<OWT, 1, 1, CHUNK, false, 1, 32, 1>, as mangled
_FWD = ['conv3d_spatial_kernelILi%dELi1ELi1ELi%dELb0ELi1ELi32ELi1EE' % oc
        for oc in ((32, 256), (16, 256), (8, 256), (8, 64))]
_BWD = ['conv3d_wgrad_ci1_bn_kernelILi1EE', 'conv3d_wgrad_ci1_bn_kernelILi2EE',
        'conv3d_wgrad_ci1_bn_finish_kernel']


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not found')
def test_stem_kernels_have_no_private_segment():
    sys.path.insert(0, os.path.join(_REPO, 'tools'))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report([os.path.join(_CSRC, 'conv3d.hip'),
                                    os.path.join(_CSRC, 'conv3d_spatial.hip')])
    for inst in _FWD + _BWD:
        hits = [k for k in rows if inst in k['mangled']]
        assert hits, f'{inst} missing from the resource report'
        for k in hits:
            assert k.get('private') == 0, kernel_resources.format_row(k)
