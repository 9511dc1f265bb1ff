"""torch.library registration of the hot-path ops (sdface-gan_amd/ops.py):
schemas, FakeTensor shape propagation and the reference's device errors, on the CPU.
The ops' results are checked on the GPU (tests/test_gpu_ops.py)."""
import ctypes
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode


@pytest.fixture(scope="module")
def ops(sdfr):
    import importlib
    return importlib.import_module(sdfr.__name__ + ".ops")


def test_ops_registered(ops):
    names = {"grid_encode_forward", "grid_encode_backward", "sh_encode_forward",
             "sh_encode_backward", "render_fused"}
    for n in names:
        assert hasattr(torch.ops.sdfr, n), n
    s = str(torch.ops.sdfr.grid_encode_forward.default._schema)
    assert s.startswith("sdfr::grid_encode_forward(Tensor inputs, Tensor embeddings, "
                        "Tensor offsets, float S")
    assert "Tensor? t_rand" in str(torch.ops.sdfr.render_fused.default._schema)


def test_grid_encode_fake_shapes(ops):
    with FakeTensorMode():
        x = torch.empty(100, 3)
        emb = torch.empty(6328848, 2)
        off = torch.empty(17, dtype=torch.int32)
        out, dy = torch.ops.sdfr.grid_encode_forward(x, emb, off, 0.533, 16, True, 0, False, 0)
        assert out.shape == (16, 100, 2) and dy.shape == (100, 96)
        out, dy = torch.ops.sdfr.grid_encode_forward(x, emb, off, 0.533, 16, False, 0, False, 0)
        assert dy.numel() == 0
        g = torch.empty(16, 100, 2)
        ge, gi = torch.ops.sdfr.grid_encode_backward(g, x, emb, off, torch.empty(100, 96), 0.533,
                                                     16, True, 0, False, 0)
        assert ge.shape == emb.shape and gi.shape == x.shape
        ge, gi = torch.ops.sdfr.grid_encode_backward(g, x, emb, off, torch.empty(0), 0.533, 16,
                                                     False, 0, False, 0)
        assert ge.numel() == 0 and gi.numel() == 0


def test_sh_encode_fake_shapes(ops):
    with FakeTensorMode():
        d = torch.empty(50, 3)
        out, dy = torch.ops.sdfr.sh_encode_forward(d, 4, True)
        assert out.shape == (50, 16) and dy.shape == (50, 48)
        gi = torch.ops.sdfr.sh_encode_backward(torch.empty(50, 16), d, dy, 4)
        assert gi.shape == d.shape


@pytest.mark.parametrize("flags,shapes", [
    (dict(output_features=1, return_sdf=1, return_xyz=1),
     [(2, 3, 8, 8), (2, 256, 8, 8), (2, 8, 8, 24, 1), (2, 1, 8, 8), (2, 3, 8, 8)]),
    (dict(output_features=1, return_sdf=0, return_xyz=0),
     [(2, 3, 8, 8), (2, 256, 8, 8), (0,), (0,), (0,)]),
])
def test_render_fused_fake_shapes(ops, sdfr, flags, shapes):
    opt = sdfr.vol_render_opt()
    ren = sdfr.VolumeFeatureRenderer(opt.rendering, style_dim=256, out_im_res=8)
    f = dict.fromkeys(ops.RENDER_FLAGS, 0)
    f.update(flags)
    ts = ren._weight_tensors(0)
    fs, is_ = ren._weight_scalars(0)
    with FakeTensorMode(allow_non_fake_inputs=True) as m:
        fake = [m.from_tensor(t.detach()) for t in ts]
        out = torch.ops.sdfr.render_fused(
            0, fake, torch.empty(2, 3, 4), torch.empty(2), torch.empty(2), torch.empty(2),
            torch.empty(2, 256), None, None, torch.empty(8), torch.empty(8), torch.empty(24),
            None, fs, is_, [f[k] for k in ops.RENDER_FLAGS], 8, 8, 24)
    assert [tuple(o.shape) for o in out] == shapes


def test_weight_tensors_order(sdfr):
    """The flat list feeds ops.weights_struct positionally: its length per network."""
    opt = sdfr.vol_render_opt()
    ren = sdfr.VolumeFeatureRenderer(opt.rendering, style_dim=256, out_im_res=8)
    assert len(ren._weight_tensors(0)) == 4 + 6 * 3 + 6 + 4 + 1
    assert ren._weight_tensors(0)[0] is ren.network.encoder.embeddings
    assert ren._weight_tensors(0)[-1] is ren.sigmoid_beta


@pytest.mark.parametrize("kind, net", [(0, dict()), (1, dict(ngp=False)),
                                       (2, dict(ngp=False, fc=True))])
def test_weight_tensors_follow_the_network_table(sdfr, kind, net):
    """The flat list is one tensor per name of _lib.NETWORKS[kind].fields, in that order,
    and weights_struct puts each into the struct member of that name."""
    ren = sdfr.VolumeFeatureRenderer(sdfr.vol_render_opt(**net).rendering, style_dim=256,
                                     out_im_res=8)
    assert ren._net_kind() == kind
    row = sdfr._lib.NETWORKS[kind]
    ts = ren._weight_tensors(kind)
    assert len(ts) == len(row.fields) == len(set(row.fields))
    assert len({t.data_ptr() for t in ts}) == len(ts)
    w = ren._weight_struct(kind)
    assert type(w) is row.weights
    for name, t in zip(row.fields, ts):
        member, _, index = name.partition("[")
        got = getattr(w, member)[int(index[:-1])] if index else getattr(w, member)
        assert got == t.data_ptr(), name
    named = dict(ren.named_parameters())
    assert ts[row.fields.index("sigma_w")] is named["network.sigma_linear.weight"]
    assert ts[row.fields.index("pts_b[2]")] is named["network.pts_linears.2.bias"]
    assert ts[row.fields.index("views_w")] is named["network.views_linears.weight"]
    assert ts[-1] is ren.sigmoid_beta and row.fields[-1] == "sigmoid_beta"
    # every tensor member of the struct is in the table
    pointers = {n if not hasattr(t, "_length_") else f"{n}[{i}]"
                for n, t in row.weights._fields_ for i in range(getattr(t, "_length_", 1))
                if t is ctypes.c_void_p or getattr(t, "_type_", None) is ctypes.c_void_p}
    assert pointers == set(row.fields)


def test_ops_raise_on_host_tensors(ops):
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        torch.ops.sdfr.grid_encode_forward(torch.zeros(4, 3), torch.zeros(10, 2),
                                           torch.zeros(17, dtype=torch.int32), 0.5, 16, False,
                                           0, False, 0)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        torch.ops.sdfr.sh_encode_forward(torch.zeros(4, 3), 4, False)
