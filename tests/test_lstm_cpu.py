"""ops.OpsLSTM and models.ICALstm without a GPU: on the CPU OpsLSTM is
nn.LSTM (same parameters, same state dict, same numbers), and the inputs the
native path hands to the library (PackedSequence, proj_size) are accepted."""
import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence

from coinstac_dinunet_amd import ops
from coinstac_dinunet_amd.models import ICALstm


@pytest.mark.parametrize('kw', [
    dict(), dict(num_layers=2, bidirectional=True, batch_first=True),
    dict(bias=False, bidirectional=True), dict(proj_size=3)], ids=str)
def test_opslstm_is_nn_lstm_on_cpu(kw):
    torch.manual_seed(0)
    stock = nn.LSTM(6, 10, **kw)
    mine = ops.OpsLSTM(6, 10, **kw)
    assert ([n for n, _ in mine.named_parameters()]
            == [n for n, _ in stock.named_parameters()])
    mine.load_state_dict(stock.state_dict())
    stock.load_state_dict(mine.state_dict())
    x = torch.randn(5, 4, 6)
    y0, (h0, c0) = stock(x)
    y1, (h1, c1) = mine(x)
    assert torch.equal(y0, y1) and torch.equal(h0, h1) and torch.equal(c0, c1)
    y2, _ = mine(x, (h1, c1))
    assert torch.equal(y2, stock(x, (h0, c0))[0])


def test_opslstm_takes_a_packed_sequence():
    torch.manual_seed(1)
    mine = ops.OpsLSTM(6, 10, bidirectional=True)
    packed = pack_padded_sequence(torch.randn(5, 3, 6), [5, 3, 2])
    y, (h, _) = mine(packed)
    assert y.data.shape == (10, 20) and h.shape == (2, 3, 10)


def test_icalstm_shape_and_one_training_step():
    torch.manual_seed(2)
    net = ICALstm(num_comps=8, window_size=4, input_size=16, hidden_size=12)
    x = torch.randn(3, 5, 8, 4)
    target = torch.tensor([0, 1, 1])
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    out = net(x)
    assert out.shape == (3, 2)
    before = ops.cross_entropy(out, target)
    before.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in net.parameters())
    opt.step()
    assert ops.cross_entropy(net(x), target) < before
    default = ICALstm()
    assert default.lstm.hidden_size == 128 and default.lstm.bidirectional
    assert default(torch.randn(2, 3, 53, 20)).shape == (2, 2)
