"""The recurrent LSTM kernels keep W_hh fragments (Hp <= 128), the cell state
and the gate accumulators in registers indexed by compile-time constants
only: no instance may carry a private segment (a spill, or a fragment array
that went to memory through a runtime index). Read from the compiler's
resource remarks via tools/kernel_resources.py (CPU, needs hipcc)."""
import os
import shutil
import sys

import pytest

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(_REPO, 'coinstac_dinunet_amd', 'ops', 'csrc', 'lstm.hip')


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not found')
def test_lstm_kernels_have_no_private_segment():
    sys.path.insert(0, os.path.join(_REPO, 'tools'))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = kernel_resources.report([_SRC])
    names = [k['name'] for k in rows]
    # register-stationary (32, 128) and streamed (160, 256) instances
    for inst in ('lstm_rec_fwd_kernel<32, true>',
                 'lstm_rec_fwd_kernel<128, true>',
                 'lstm_rec_fwd_kernel<128, false>',
                 'lstm_rec_fwd_kernel<160, true>',
                 'lstm_rec_fwd_kernel<256, true>',
                 'lstm_rec_fwd_kernel<256, false>',
                 'lstm_rec_bwd_kernel<32>', 'lstm_rec_bwd_kernel<128>',
                 'lstm_rec_bwd_kernel<160>', 'lstm_rec_bwd_kernel<256>'):
        assert inst in names, f'{inst} missing from the resource report'
    bad = [kernel_resources.format_row(k) for k in rows
           if k.get('private') != 0]
    assert not bad, 'lstm kernels with a private segment:\n' + '\n'.join(bad)
