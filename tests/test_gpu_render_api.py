"""GPU: the split-fp16 calls with the weights packed inside the call's workspace
(``prepacked == NULL``) against the same calls on weights packed beforehand, which is what
the Python paths always pass.  Both run the same kernels on the same packing, so every
output is equal bit for bit."""
import pytest
import torch

from tests.golden import weights as W
from tests.test_gpu_fc import make_fc
from tests.test_gpu_geometry import _cameras
from tests.test_gpu_render import DEV, make_renderer, make_siren
from tests.test_gpu_siren_query import _generic_points

pytestmark = pytest.mark.gpu

RES, B = 8, 2
CALLS = ["render_ngp", "render_siren", "render_fc", "query_ngp", "grad_ngp", "geometry_ngp"]


def _renderer(sdfr, golden_dir, call):
    kind = call.split("_")[1]
    flags = dict(return_sdf=True, return_xyz=True)
    if kind == "ngp":
        sd = W.det_state_dict(W.golden_entries(golden_dir), "renderer.")
        return make_renderer(sdfr, sd, RES, 24, **flags)
    sd = W.det_state_dict(W.golden_entries(golden_dir, kind=kind), "renderer.")
    return (make_siren if kind == "siren" else make_fc)(sdfr, sd, RES, 24, **flags)


def _run(ren, call, sdfr):
    cam, focal, near, far, lat, tr = _cameras(sdfr, RES, B, 7)
    pts, dirs = (torch.from_numpy(t).to(DEV) for t in _generic_points())
    with torch.no_grad():
        if call.startswith("render"):
            assert ren._fused_ok(cam, lat, False)
            out = ren(cam, focal, near, far, styles=lat, t_rand=tr)
        elif call == "query_ngp":
            assert ren._query_fused_ok(pts, lat)
            out = ren.query(pts, lat, viewdirs=dirs)
        elif call == "grad_ngp":
            assert ren._query_fused_ok(pts, lat)
            out = ren.query_gradient(pts, lat)
        else:
            assert ren._query_fused_ok(cam, lat)
            out = ren.render_geometry(cam, focal, near, far, lat, t_rand=tr)
    torch.cuda.synchronize()
    return [t for t in out if torch.is_tensor(t)]


@pytest.mark.parametrize("call", CALLS)
def test_packing_in_the_workspace_equals_prepacked(sdfr, golden_dir, monkeypatch, call):
    ren = _renderer(sdfr, golden_dir, call)
    want = _run(ren, call, sdfr)
    asked = []
    monkeypatch.setattr(ren, "_prepacked", lambda *a, **k: asked.append(a))
    got = _run(ren, call, sdfr)
    assert asked, "the call did not ask for packed weights"
    assert len(got) == len(want) >= 2
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g, w)
