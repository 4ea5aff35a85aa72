"""CPU-side checks of MHTransformerConv (no GPU): the restated PyG convolution the fixtures are generated with, construction and
state-dict layout of the models, the packed operand layout of the fused kernel, and the ABI entries' argument checks."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden


def _graph(n=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, 6 * n), generator=g)
    ei = torch.cat([ei, torch.arange(n).repeat(2, 1)], dim=1)          # every node has an incoming edge
    return ei, torch.rand(ei.shape[1], 2, generator=g), torch.Generator().manual_seed(seed + 1)


def test_restatement_single_head_equals_oracle_transformer_conv():
    from mh_restated import TransformerConv
    from oracle import qt_oracle as O
    ei, ea, g = _graph()
    conv = TransformerConv(6, 8, 1, False, False, 0.0, 2)
    for p in conv.parameters():
        p.data.normal_(0, 0.5, generator=g)
    x = torch.randn(40, 6, generator=g)
    want = O.transformer_conv(x, ei, ea, dict(conv.named_parameters()))
    assert torch.allclose(conv(x, ei, ea), want, rtol=1e-6, atol=1e-6)
    assert [k for k, _ in conv.named_parameters()] == [k for k, _ in O.TransformerConv(6, 8).named_parameters()]


@pytest.mark.parametrize('h', [8, 16, 32])
def test_seq2seq_builds_with_mhtransformerconv(h):
    from model.model import MHTransformerConv
    from model.seq2seq import Seq2Seq
    m = Seq2Seq(h, 0.1, 0.15, input_features=6, n_layers=1, n_conv_layers=2, convolution_type='MHTransformerConv')
    assert type(m.decoder.fc_out1) is MHTransformerConv and type(m.encoder.rnns[0].conv_x_i.convolutions[0]) is MHTransformerConv
    assert m.decoder.fc_out1.heads == 3 and m.decoder.fc_out1.dropout == 0.1 and m.decoder.fc_out2.out_channels == 1
    assert m.use_edge_attrs


@pytest.mark.parametrize('h', [12, 64])
def test_seq2seq_refuses_unbuilt_hidden_sizes(h):
    from model.seq2seq import Seq2Seq
    with pytest.raises(ValueError, match='hidden_size'):
        Seq2Seq(h, 0.1, 0.15, convolution_type='MHTransformerConv')


def test_state_dict_layout_matches_reference():
    """Keys (in order) and shapes of the reference's Seq2Seq with MHTransformerConv (mh_rollout.npz, written by the reference)."""
    from model.seq2seq import Seq2Seq
    g = golden('mh_rollout.npz')
    m = Seq2Seq(8, 0.0, 0.15, input_timesteps=2, input_features=6, output_timesteps=3, n_layers=1, n_conv_layers=2,
                convolution_type='MHTransformerConv')
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['keys']]
    for (k, v), s in zip(sd.items(), g['shapes']):
        assert list(v.shape) == [int(d) for d in s[:v.dim()]] and not s[v.dim():].any(), k
    assert [k for k, _ in m.named_parameters()] == [k[2:] for k in g.files if k.startswith('g/')]


def _packed_reference(pc, x, ei, ea, cout, H):
    """The arithmetic of qt_mhattn_fwd on the packed operands, in torch: proj = [x | 1] W, per head softmax attention over the
    edges, cat (N, H cp), y = cat Wt + blin."""
    n, cp = x.shape[0], pc.Wt.shape[1]
    xin = F.pad(x, (0, pc.W.shape[0] - 4 - x.shape[1]))
    proj = (xin @ pc.W[:-4] + pc.W[-4]).view(n, H, 4, cp)
    q, k, v, sk = proj.unbind(2)
    src, dst = ei
    e = torch.einsum('ea,hca->ehc', ea, pc.We)
    a = (q[dst] * (k[src] + e)).sum(-1) / math.sqrt(cout)
    idx = dst.unsqueeze(1).expand(-1, H)
    amax = torch.full((n, H), -float('inf')).scatter_reduce(0, idx, a, 'amax', include_self=True)
    ex = torch.exp(a - amax[dst])
    alpha = ex / torch.zeros(n, H).index_add(0, dst, ex)[dst]
    cat = torch.zeros(n, H, cp).index_add(0, dst, alpha.unsqueeze(-1) * (v[src] + e)) + sk
    return cat.reshape(n, H * cp) @ pc.Wt + pc.bl


@pytest.mark.parametrize('cin,cout', [(6, 8), (8, 1), (9, 16), (32, 32)])
def test_packed_layout_reproduces_restated_convolution(cin, cout):
    """The matrices MHTransformerConv.pack_many hands the kernel (head-major [q | k | v | skip] rows, We per head, Wlin^T split by
    head, zero padding above out_channels) give the restated convolution + head merge, with the reference module's weights."""
    import mh_restated
    from model.model import CONVOLUTION_KWARGS, MHTransformerConv
    ei, ea, g = _graph(seed=cin + cout)
    kw = CONVOLUTION_KWARGS['MHTransformerConv']
    mine = MHTransformerConv(cin, cout, **kw)
    ref = mh_restated.TransformerConv(cin, cout, kw['heads'], True, False, kw['dropout'], kw['edge_dim'])
    lin = torch.nn.Linear(kw['heads'] * cout, cout)
    with torch.no_grad():
        for p in list(ref.parameters()) + list(lin.parameters()):
            p.normal_(0, 0.4, generator=g)
    sd = dict(ref.state_dict(), **{'lin.' + k: v for k, v in lin.state_dict().items()})
    mine.load_state_dict(sd)
    assert list(mine.state_dict().keys()) == list(sd.keys())
    ref.eval()
    x = torch.randn(40, cin, generator=g)
    want = lin(ref(x, ei, ea))
    pc, pc2 = MHTransformerConv.pack_many([mine, mine])
    assert torch.equal(pc.W, pc2.W) and pc.acc is not pc2.acc
    got = _packed_reference(pc, x, ei, ea, cout, kw['heads'])
    np.testing.assert_allclose(got[:, :cout].detach().numpy(), want.detach().numpy(), rtol=1e-5, atol=1e-5)
    assert not got[:, cout:].any()                                     # padding columns of y stay zero


def test_mh_abi_entries_refuse_null_arguments():
    from qtmpnn import _lib
    lib = _lib.load()
    calls = {
        'qt_mhattn_fwd': (None,) * 8 + (8, 8, 3, 4, None, 1.0, 0, None, None, None, None, None),
        'qt_mhattn_bwd_merge': (None, 8, None, None, 8, 3, 4, None, None, None, 0, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
        assert name.encode() in lib.qt_last_error(), (name, lib.qt_last_error())
    x = ctypes_buf()
    # a head count or channel count the kernels are not built for is refused by name as well
    assert lib.qt_mhattn_bwd_merge(x, 8, x, x, 8, 5, 4, None, x, x, 0, None) == -1
    assert b'qt_mhattn_bwd_merge' in lib.qt_last_error()
    assert lib.qt_mhattn_fwd(*(x,) * 8, 12, 8, 3, 4, None, 1.0, 0, None, x, x, None, None) == -1
    assert b'qt_mhattn_fwd' in lib.qt_last_error()
    assert lib.qt_mhattn_blocks(1000, 8, 3) >= 1 and lib.qt_mhattn_blocks(1000, 8, 5) == 0 and lib.qt_mhattn_blocks(0, 8, 3) == 0


def ctypes_buf():
    """A host address that is only ever validated, never dereferenced (the calls above fail their argument checks first)."""
    import ctypes
    global _BUF
    _BUF = (ctypes.c_float * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_unbuilt_variants_still_raise():
    from model.seq2seq import Seq2Seq
    with pytest.raises(NotImplementedError):
        Seq2Seq(16, 0.1, 0.1, convolution_type='GATv2Conv')
