"""The attention kernels keep the Q / K / V / dO fragments, the score tiles
and every accumulator in registers indexed by compile-time constants only: no
instance may carry a private segment. Read from the compiler's resource
remarks via tools/kernel_resources.py (CPU, needs hipcc)."""
import os
import shutil
import sys

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_REPO, 'coinstac_dinunet_amd', 'ops', 'csrc',
                    'attention.hip')


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not found')
def test_attention_kernels_have_no_private_segment():
    sys.path.insert(0, os.path.join(_REPO, 'tools'))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report([_SRC])
    names = [k['name'] for k in rows]
    for kern in ('attn_fwd_kernel', 'attn_bwd_dkv_kernel',
                 'attn_bwd_dq_kernel'):
        for dtype in ('float', 'c10::BFloat16'):
            for dp in (32, 64, 128):
                inst = f'{kern}<{dtype}, {dp}>'
                assert inst in names, f'{inst} missing from the report'
    bad = [kernel_resources.format_row(k) for k in rows
           if k.get('private') != 0 or k.get('lds', 0) > 64 * 1024]
    assert not bad, ('attention kernels with a private segment or more than '
                     '64 KB of LDS:\n' + '\n'.join(bad))
