"""Host-side checks of the attention-coefficient feature: the ABI entry's argument checks, the call signatures existing callers use,
the recording block's refusals, the restated coefficients (tests/attn_restated.py) and the fixture's records."""
import inspect
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _buf():
    """A 16-byte aligned host address that is only ever validated, never dereferenced (the calls fail their argument checks first)."""
    import ctypes
    global _BUF
    _BUF = (ctypes.c_float * 64)()
    return ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 16


def test_attn_weights_abi_refuses_bad_arguments_by_name():
    from qtmpnn import _lib
    lib = _lib.load()
    x = _buf()

    def call(proj=x, ld=32, ps=0, hs=0, C=8, c_real=8, G=1, N=10, rev=x, ae=x, as_=x, rowptr=x):
        return lib.qt_attn_weights(rowptr, x, x, None, proj, ld, ps, hs, x, C, c_real, G, N, None, rev, 20, ae, as_, None)

    for kw in (dict(proj=None), dict(rev=None), dict(ae=None), dict(as_=None), dict(rowptr=None),     # NULL operands
               dict(C=64, c_real=8, ld=256), dict(C=12, c_real=12, ld=48), dict(C=8, c_real=9),      # channel counts not built
               dict(G=0), dict(G=65),                                                                 # group count
               dict(ld=30), dict(ps=6), dict(hs=34), dict(proj=x + 4)):                               # strides / alignment
        assert call(**kw) == -1, kw
        assert b'qt_attn_weights' in lib.qt_last_error(), (kw, lib.qt_last_error())
    assert call(N=0) == 0            # nothing to do: no launch


def test_existing_call_signatures_are_kept():
    """The keyword comes after `packed`: every positional and keyword call of the convolutions is unchanged."""
    from model.model import MHTransformerConv, TransformerConv
    for cls in (TransformerConv, MHTransformerConv):
        ps = list(inspect.signature(cls.forward).parameters.values())
        assert [p.name for p in ps] == ['self', 'x', 'edge_index', 'edge_weight', 'packed', 'return_attention_weights']
        assert all(p.default is None for p in ps[3:])


def test_flag_given_twice_or_not_a_bool_is_refused():
    from model.model import TransformerConv
    conv = TransformerConv(4, 8)
    with pytest.raises(TypeError, match='given twice'):
        conv(torch.zeros(3, 4), None, None, True, return_attention_weights=True)
    with pytest.raises(TypeError, match='bool'):
        conv(torch.zeros(3, 4), None, return_attention_weights='yes')


def _model(conv='TransformerConv'):
    from model.seq2seq import Seq2Seq
    return Seq2Seq(hidden_size=8, dropout=0.0, thresh=0.1, input_timesteps=2, input_features=4, output_timesteps=2, n_layers=1,
                   n_conv_layers=2, convolution_type=conv)


def test_record_attention_refuses_static_mode_and_nesting():
    from model import model as M
    model = _model()
    model.static_shapes = True
    with pytest.raises(RuntimeError, match='static mode'):
        with model.record_attention():
            pass
    assert M._RECORDER[0] is None
    model.static_shapes = False
    with model.record_attention() as rec:
        assert M._RECORDER[0] is not None and rec == []
        with pytest.raises(RuntimeError, match='nest'):
            with model.record_attention():
                pass
    assert M._RECORDER[0] is None


def test_recorder_selects_attention_convolutions_by_name_or_predicate():
    from model.model import AttentionRecorder
    model = _model('MHTransformerConv')
    every = AttentionRecorder(model)
    convs = [m for _, m in model.named_modules() if type(m).__name__ == 'MHTransformerConv']
    assert len(convs) == 16 + 8 + 2 and all(every.name_of(c) for c in convs)
    assert every.name_of(model.decoder.fc_out2) == 'decoder.fc_out2'
    assert every.name_of(model.encoder.rnns[0].conv_h_c.convolutions[1]) == 'encoder.rnns.0.conv_h_c.convolutions.1'
    one = AttentionRecorder(model, ['decoder.fc_out1'])
    assert [c for c in convs if one.name_of(c)] == [model.decoder.fc_out1]
    pred = AttentionRecorder(model, lambda n: n.startswith('encoder.'))
    assert sum(bool(pred.name_of(c)) for c in convs) == 16


def test_restated_coefficients_sum_to_one_and_rebuild_the_output():
    from attn_restated import coefficients
    import mh_restated
    torch.manual_seed(2)
    n = 7
    src = torch.tensor([0, 1, 1, 2, 3, 4, 5, 6, 6, 0, 3, 3])
    dst = torch.tensor([1, 0, 2, 1, 4, 3, 6, 5, 0, 6, 3, 2])
    ei, ea = torch.stack([src, dst]), torch.rand(12, 2)
    for H, concat in ((1, False), (3, True)):
        conv = mh_restated.TransformerConv(5, 4, heads=H, concat=concat, edge_dim=2).eval()
        x = torch.randn(n, 5)
        a = coefficients(conv, x, ei, ea).detach()
        assert a.shape == (12, H)
        np.testing.assert_allclose(torch.zeros(n, H).index_add(0, dst, a).numpy(), np.ones((n, H)), rtol=1e-6)
        with torch.no_grad():
            v, e = conv.lin_value(x).view(n, H, 4), conv.lin_edge(ea).view(-1, H, 4)
            agg = torch.zeros(n, H, 4).index_add(0, dst, a.unsqueeze(-1) * (v[src] + e))
            out = (agg.reshape(n, H * 4) if concat else agg.mean(1)) + conv.lin_skip(x)
            np.testing.assert_allclose(out.numpy(), conv(x, ei, ea).numpy(), rtol=1e-5, atol=1e-6)


def test_fixture_records_are_unique_and_cover_the_rollout():
    """attn_rollout.npz: one record per (name, t), names of this project's Seq2Seq, every attention convolution of the reference's
    forward at every step of its phase (2 encoder and 2 decoder steps), edges sorted like Mesh.edge_index, alpha summing to 1."""
    g = np.load(os.path.join(GOLDEN, 'attn_rollout.npz'))
    n = int(g['n_records'])
    keys = [(str(g[f'name_{i}']), int(g[f't_{i}'])) for i in range(n)]
    assert len(set(keys)) == n
    model = _model()
    convs = [nm for nm, m in model.named_modules() if type(m).__name__ == 'TransformerConv']
    assert len(convs) == 16 + 8 + 2
    assert set(keys) == {(nm, t) for nm in convs for t in range(2)}
    for i in range(n):
        e, a = g[f'edges_{i}'], g[f'alpha_{i}']
        assert e.dtype == np.int32 and a.dtype == np.float32 and a.shape == (e.shape[1], 1)
        key = e[0].astype(np.int64) * (e.max() + 1) + e[1]
        assert (np.diff(key) > 0).all()
        np.testing.assert_allclose(np.bincount(e[1], weights=a[:, 0]), 1.0, rtol=1e-5)
