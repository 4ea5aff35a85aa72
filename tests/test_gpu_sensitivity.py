"""NextFramePredictorS2S.sensitivity on the GPU against the float64 oracle (tests/sensitivity_cases.py: oracle.qt_oracle.Seq2Seq on
the CPU in float64 with the same weights on the same meshes, J_t formed there, the maps from torch.autograd.grad with respect to
its input) -- never against the code under test.  32 x 32 frames, T_in = 3, T_out = 2, hidden 8, dropout 0, eval mode, two
different clips: the smallest shapes with several quadtree levels, a mask and two clips.

The bound is tests/helpers.py::grad_close per (clip, lead) map -- rtol 1e-4 with an absolute floor of 5e-5 x the map's largest
entry (floor=0: the maps' entries are of order 1e-3 and smaller, the helper's default floor of 1e-3 would widen the bound).
Every comparison prints its two figures (worst error over the map's largest entry; worst ratio to the bound) before it asserts;
profiles/sensitivity.txt holds a recorded run, beside the same figures of the oracle evaluated in float32.  Measured on one
MI355X, worst ratio to the bound, GPU (float32 oracle): ChebConv preset 0.053 (0.087), with a region target 0.096 (0.132); GCNConv
pixelwise 0.006 (0.003); TransformerConv 0.009 (0.007); MHTransformerConv 0.002 (0.005); ChebConv on data-driven meshes 0.795
(0.301), worst error 7.4e-5 of the map's largest entry; integrated gradients 0.086 (0.166).  No case needs more than grad_close."""
import numpy as np
import pytest
import torch

import sensitivity_cases as S
from helpers import close, dev, grad_close

pytestmark = pytest.mark.gpu
LEADS = (0, 1)


class Case:
    """One case built once: the oracle, the predictor with its weights, the inputs, and the mesh arguments of both sides."""

    def __init__(self, name, monkeypatch):
        from model.graph_functions import create_static_heterogeneous_graph
        from model.model import CONVOLUTION_KWARGS
        from model.mpnnlstm import NextFramePredictorS2S
        c = self.c = S.CASES[name]
        self.name = name
        self.ref = S.oracle_model(name, monkeypatch)
        if 'heads' in c:
            monkeypatch.setitem(CONVOLUTION_KWARGS[c['conv']], 'heads', c['heads'])
        self.nfp = NextFramePredictorS2S(thresh=c['thresh'], input_features=c['cin'], input_timesteps=S.T_IN,
                                         output_timesteps=S.T_OUT, device=dev(),
                                         model_kwargs=dict(hidden_size=S.HIDDEN, dropout=0.0, n_layers=c['nl'],
                                                           n_conv_layers=c['nc'], convolution_type=c['conv']))
        self.nfp.model.load_state_dict(self.ref.state_dict())
        self.nfp.model.to(dev()).eval()
        self.x, self.concat = S.inputs(name)
        self.mask = S.land_mask()
        self.hir = S.high_interest() if c['mesh'] != 'pixel' else None
        attn = c['conv'] in ('TransformerConv', 'MHTransformerConv')
        self.gs = self.gsr = None
        if c['mesh'] == 'preset':
            self.gs = create_static_heterogeneous_graph(S.SHAPE, 8, self.mask, high_interest_region=self.hir, use_edge_attrs=attn,
                                                        device=dev())
            mesh = self.gs['mapping']
            assert mesh.N > 64 and len(set(mesh.npix.cpu().tolist())) >= 3, 'several quadtree levels'
            self.gsr = dict(labels=mesh.labels[0].cpu().numpy(), n_pixels_per_node=mesh.npix.cpu().double(),
                            edge_index=mesh.edge_index(True).cpu(), edge_attrs=mesh.edge_attrs(attn).cpu().double())
        self.fwd = dict(mask=self.mask, graph_structure=self.gs, **({'high_interest_region': self.hir} if c['mesh'] == 'data' else {}))
        self.xt, self.ct = torch.from_numpy(self.x).to(dev()), torch.from_numpy(self.concat).to(dev())

    def oracle(self, target=None, dtype=torch.float64):
        return S.oracle_gradient(self.ref, self.x, self.concat, S.weights_of(target, self.mask), LEADS, dtype, self.mask,
                                 self.hir if self.c['mesh'] == 'data' else None, self.gsr)

    def sensitivity(self, **kw):
        return self.nfp.sensitivity(self.xt, self.ct, leads=LEADS, **self.fwd, **kw)


def report(tag, got, ref):
    rel, ratio = S.distance(got, ref)
    print(f'sensitivity {tag}: worst |got - ref| / max|ref| = {rel:.3e}, worst ratio to the grad_close bound = {ratio:.3f}')
    return rel, ratio


def check_maps(tag, got, ref):
    """grad_close on every (clip, lead) map, after the figures are printed."""
    report(tag, got, ref)
    assert got.shape == ref.shape
    for b in range(ref.shape[0]):
        for l in range(ref.shape[1]):
            grad_close(got[b, l], ref[b, l], rtol=S.RTOL, rel_atol=S.REL_ATOL, floor=0.0, msg=f'{tag}: clip {b}, lead {LEADS[l]}')


def check_result(s, B, method='gradient'):
    assert s.maps.dtype == np.float32 and s.maps.shape[:2] == (B, len(LEADS)) and s.leads == LEADS and s.method == method
    assert s.J.dtype == np.float64 and s.J.shape == (B, len(LEADS)) and np.isfinite(s.maps).all()


@pytest.mark.parametrize('target', ['default', 'region'])
def test_chebconv_preset_mesh_gradient(monkeypatch, target):
    """Case 1: ChebConv, 2 layers x 2 conv layers, preset heterogeneous mesh with a land mask, one input channel; 'gradient' at
    both leads with the default target and with a rectangular region."""
    case = Case('cheb_preset', monkeypatch)
    w = None if target == 'default' else S.region_target()
    J, maps, _ = case.oracle(w)
    s = case.sensitivity(target=w)
    check_result(s, S.B)
    close(s.J, J, msg='J')
    check_maps(f'cheb_preset/{target}', s.maps, maps)
    assert np.array_equal(s.target, S.weights_of(w, case.mask))
    assert not s.maps[..., case.mask, :].any(), 'pixels under the mask reach no node: their sensitivity is exactly 0'


def test_gcnconv_pixelwise_mesh_four_channels(monkeypatch):
    """Case 2: GCNConv on the pixelwise mesh (thresh = -inf) with a mask and four input channels: the channel axis of the maps
    and the zero-padded feature columns (4 + 3 channels padded to 8)."""
    case = Case('gcn_pixel', monkeypatch)
    J, maps, _ = case.oracle()
    s = case.sensitivity()
    check_result(s, S.B)
    assert s.maps.shape[-1] == 4 and all(np.abs(s.maps[..., c]).max() > 0 for c in range(4))
    close(s.J, J, msg='J')
    check_maps('gcn_pixel', s.maps, maps)


@pytest.mark.parametrize('name', ['transformer_preset', 'mh_preset'])
def test_attention_stacks_preset_mesh(monkeypatch, name):
    """Case 3: TransformerConv and MHTransformerConv (2 heads) with edge attributes on a preset mesh."""
    case = Case(name, monkeypatch)
    J, maps, _ = case.oracle()
    s = case.sensitivity()
    check_result(s, S.B)
    close(s.J, J, msg='J')
    check_maps(name, s.maps, maps)


def test_chebconv_data_driven_meshes(monkeypatch):
    """Case 4: ChebConv on data-driven quadtree meshes: the decoder re-meshes on its own output, so the maps pass through the
    state transfer between meshes.  The label maps of every step equal the oracle's bit for bit first (the meshes are then the
    same on both sides and held fixed on both); then the maps are compared."""
    case = Case('cheb_data', monkeypatch)
    J, maps, labels = case.oracle()
    with torch.no_grad():
        _, meshes = case.nfp.model(case.xt, concat_layers=case.ct, teacher_forcing_ratio=0, **case.fwd)
    for t, ms in enumerate(meshes):
        off = ms.node_off.cpu().numpy()
        for b in range(S.B):
            lab = ms.labels[b].cpu().numpy()              # (the batched mesh numbers its nodes clip after clip)
            assert np.array_equal(np.where(lab >= 0, lab - off[b], -1), labels[b][t]), f'labels of step {t}, clip {b}'
    assert any(not np.array_equal(labels[b][0], labels[b][1]) for b in range(S.B)), 'the decoder re-meshed'
    s = case.sensitivity()
    check_result(s, S.B)
    close(s.J, J, msg='J')
    check_maps('cheb_data', s.maps, maps)


def test_integrated_gradients_and_gradient_x_input(monkeypatch):
    """Case 5: 'integrated' with steps = 4 on case 1 against the oracle evaluated at the same four midpoints (formed in
    float32 as the product forms them), with a non-zero baseline; J and J_baseline against the oracle's values.  completeness():
    the oracle's own residual at 4 points is the midpoint rule's error, not zero; the two residuals are sums of the maps minus
    (J - J_baseline), so their difference is held to the sum of the map bound over a map's entries plus the bound of the two J
    values -- what the entrywise bounds allow, no fixed number.  'gradient_x_input' against the oracle's product."""
    case = Case('cheb_preset', monkeypatch)
    w = S.weights_of(None, case.mask)
    base = np.full_like(case.x[0], 0.05)
    for tag, baseline, base_b in (('zero baseline', None, np.zeros_like(case.x)), ('baseline 0.05', base, np.stack([base] * S.B))):
        J, Jb, maps, res = S.oracle_integrated(case.ref, case.x, base_b, case.concat, w, LEADS, 4, torch.float64, case.mask, None, case.gsr)
        s = case.sensitivity(method='integrated', steps=4, baseline=baseline)
        check_result(s, S.B, 'integrated')
        close(s.J, J, msg='J')
        close(s.J_baseline, Jb, msg='J_baseline')
        check_maps(f'integrated/{tag}', s.maps, maps)
        got = s.completeness()
        entry = S.RTOL * np.abs(maps) + S.REL_ATOL * np.abs(maps).max(axis=(2, 3, 4, 5), keepdims=True)
        bound = entry.sum(axis=(2, 3, 4, 5)) + 2 * 1e-5 + 1e-4 * (np.abs(J) + np.abs(Jb))
        print(f'sensitivity integrated/{tag}: residual (oracle) {res.ravel()}, (GPU) {got.ravel()}, bound on the difference {bound.ravel()}')
        assert np.abs(res).max() > 0 and (np.abs(got - res) <= bound).all()
    _, grads, _ = case.oracle()
    s = case.sensitivity(method='gradient_x_input', baseline=base)
    check_result(s, S.B, 'gradient_x_input')
    check_maps('gradient_x_input', s.maps, grads * (case.x.astype(np.float64) - base)[:, None])


def test_batched_call_equals_single_calls(monkeypatch):
    """Case 6: sensitivity on B = 2 equals two B = 1 calls under the fp32 bound, and an unbatched x returns B = 1.  The equality
    was bit for bit when measured on one MI355X (printed by every run): the meshes are block diagonal, no sum of the data
    path crosses a clip, and the batched launches reduced a clip's rows in the order the single-clip launches do.  The
    assertion is the fp32 bound all the same: the order of a reduction inside a launch is not part of any contract."""
    case = Case('cheb_preset', monkeypatch)
    both = case.sensitivity()
    singles = [case.nfp.sensitivity(case.xt[b], case.ct[b], leads=LEADS, **case.fwd) for b in range(S.B)]
    for b, one in enumerate(singles):
        check_result(one, 1)
        print(f'sensitivity batched vs single, clip {b}: bit for bit = {np.array_equal(one.maps[0], both.maps[b])}')
        check_maps(f'batched vs single, clip {b}', both.maps[b:b + 1], one.maps.astype(np.float64))
        close(both.J[b], one.J[0])
    one = case.nfp.sensitivity(case.xt[:1], case.ct[:1], leads=(1,), **case.fwd)
    assert one.maps.shape == (1, 1, S.T_IN, *S.SHAPE, 1) and one.leads == (1,)
    check_maps('lead 1 alone', one.maps, both.maps[:1, 1:].astype(np.float64))


def _trained(monkeypatch, name):
    case = Case(name, monkeypatch)
    case.nfp.initiate_training(lr=1e-3, lr_decay=0.95)
    case.nfp.model.train()
    return case


@pytest.mark.parametrize('name', ['cheb_preset', 'gcn_pixel'])
def test_no_side_effects_on_training(monkeypatch, name):
    """Case 7: after one train_step, sensitivity (in eval mode) leaves every param.grad (the flat gradient vector on the packed
    ChebConv model), the optimiser state, requires_grad, static_shapes and the mode bit-equal, and a second train_step then
    gives the loss bits and weights of a twin that never called it; a predictor that never trained keeps grad = None."""
    from qtmpnn.optim import adam_state
    a, twin = _trained(monkeypatch, name), _trained(monkeypatch, name)
    assert (a.nfp.flat is not None) == (name == 'cheb_preset')
    y = torch.from_numpy(np.random.default_rng(3).random((S.B, S.T_OUT, *S.SHAPE, 1)).astype(np.float32)).to(dev())
    step = lambda c: c.nfp.train_step(c.xt, y, c.ct, c.mask, graph_structure=c.gs)
    assert torch.equal(step(a), step(twin))
    params = list(a.nfp.model.parameters())
    snap = lambda t: None if t is None else t.detach().clone()

    def state():
        flat = a.nfp.flat
        return dict(grads=[snap(p.grad) for p in params], ptrs=[None if p.grad is None else p.grad.data_ptr() for p in params],
                    flat_grad=None if flat is None else snap(flat.param.grad), vector=None if flat is None else snap(flat.grad_vector()),
                    adam=adam_state(a.nfp.optimizer, a.nfp.model), req=[p.requires_grad for p in params],
                    flat_req=None if flat is None else flat.param.requires_grad, static=a.nfp.model.static_shapes,
                    training=a.nfp.model.training, weights=[snap(p) for p in params])

    def same(u, v):
        if torch.is_tensor(u):
            return torch.is_tensor(v) and u.dtype == v.dtype and torch.equal(u, v)
        if isinstance(u, dict):
            return u.keys() == v.keys() and all(same(u[k], v[k]) for k in u)
        if isinstance(u, (list, tuple)):
            return len(u) == len(v) and all(same(p, q) for p, q in zip(u, v))
        return u == v
    for c in (a, twin):
        c.nfp.model.eval()
    before = state()
    assert any(g is not None for g in before['grads']) and (name != 'cheb_preset' or before['vector'] is not None)
    for kw in (dict(), dict(method='integrated', steps=2)):
        s = a.sensitivity(**kw)
        assert np.abs(s.maps).max() > 0
        after = state()
        for k in before:
            assert same(before[k], after[k]), k
    for c in (a, twin):
        c.nfp.model.train()
    la, lt = step(a), step(twin)
    assert torch.equal(la, lt), (float(la), float(lt))
    for p, q in zip(a.nfp.model.parameters(), twin.nfp.model.parameters()):
        assert torch.equal(p, q)
    fresh = Case(name, monkeypatch)
    fresh.sensitivity()
    assert all(p.grad is None and p.requires_grad for p in fresh.nfp.model.parameters())
    flat = fresh.nfp.model.__dict__.get('_flat_params')
    assert flat is None or (flat.param.grad is None and flat.last_grad is None and flat.param.requires_grad)


WEIGHT_GRADIENT_LAUNCHES = ('qt_wgrad', 'qt_wgrad_group', 'qt_wgrad_groups', 'qt_colsum')


def _recorded(monkeypatch):
    from qtmpnn import _lib
    launched, call = [], _lib.call

    def recorder(name, *args):
        launched.append(name)
        return call(name, *args)
    monkeypatch.setattr(_lib, 'call', recorder)
    return launched


@pytest.mark.parametrize('name', ['cheb_preset', 'gcn_pixel', 'transformer_preset', 'mh_preset'])
def test_no_weight_gradient_launches(monkeypatch, name):
    """Case 8: with no parameter requiring a gradient the weight-gradient launches and the reductions of parameter-gradient
    partials (qt_colsum) do not run, for the Chebyshev / GCN models and for the attention stacks alike: every Function on the
    path has the flag.  What cannot be dropped without changing a kernel: qt_attn_bwd and qt_mhattn_bwd_merge still form the
    per-block partial sums of lin_edge's and the head merge's gradients inside the launch that computes the data gradient, and
    the cell and head backward launches those of the peepholes, biases and LayerNorms; nothing reduces or returns them here
    ("Input sensitivities").  The same rollout with the parameters requiring gradients does launch them."""
    case = Case(name, monkeypatch)
    launched = _recorded(monkeypatch)
    case.sensitivity()
    print(f'sensitivity launches, {name}: ' + ', '.join(f'{k} x{launched.count(k)}' for k in sorted(set(launched))))
    assert launched and not [k for k in launched if k in WEIGHT_GRADIENT_LAUNCHES]
    assert 'qt_proj_bwd' not in launched
    del launched[:]
    outs, _ = case.nfp.model(case.xt, concat_layers=case.ct, teacher_forcing_ratio=0, **case.fwd)
    sum(o.sum() for o in outs).backward()
    assert 'qt_colsum' in launched and any(k in launched for k in WEIGHT_GRADIENT_LAUNCHES[:3])


def test_refusals_on_the_device_come_before_any_launch(monkeypatch):
    """Case 9: a remesh_input=True model (NotImplementedError), static mode (RuntimeError) and a target that is zero on every
    unmasked pixel (ValueError), each before any launch."""
    from model.mpnnlstm import NextFramePredictorS2S
    case = Case('cheb_data', monkeypatch)
    remesh = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=S.T_IN, output_timesteps=S.T_OUT, device=dev(),
                                   remesh_input=True, model_kwargs=dict(hidden_size=S.HIDDEN, dropout=0.0, n_layers=1))
    launched = _recorded(monkeypatch)
    with pytest.raises(NotImplementedError, match='sensitivity'):
        remesh.sensitivity(torch.cat([case.xt, case.xt[:, :1]], dim=1), case.ct, mask=case.mask)
    case.nfp.model.static_shapes = True
    try:
        with pytest.raises(RuntimeError, match='sensitivity'):
            case.sensitivity()
    finally:
        case.nfp.model.static_shapes = False
    only_masked = case.mask.astype(np.float32)
    with pytest.raises(ValueError, match='target: the weights of the unmasked pixels sum to 0'):
        case.sensitivity(target=only_masked)
    with pytest.raises(RuntimeError, match='x must live on the GPU'):
        case.nfp.sensitivity(case.xt.cpu(), case.ct, leads=LEADS, **case.fwd)
    assert launched == []
    assert np.abs(case.sensitivity().maps).max() > 0 and launched
