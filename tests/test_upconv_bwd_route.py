"""route_upconv3d_bwd is a pure function of the shape, importable without a
GPU."""
from coinstac_dinunet_amd.ops.conv import route_upconv3d_bwd


def test_route_upconv3d_bwd(monkeypatch):
    monkeypatch.delenv('COINN_UPCONV_BWD', raising=False)
    assert route_upconv3d_bwd(64, 32, 16, 16) == 'collapsed'
    assert route_upconv3d_bwd(8, 16, 5, 6) == 'composed'
    monkeypatch.setenv('COINN_UPCONV_BWD', 'composed')
    assert route_upconv3d_bwd(64, 32, 16, 16) == 'composed'
