"""Parameter groups on the GPU (set_param_groups, train(param_groups=)).  Two oracles: the TWIN, a deep copy of the predictor that
knows nothing of the setting and runs the plain step -- entries with (lr_scale, weight_decay) = (1, 0) must have its bits after one
step from equal state --, and the float64 model of tests/groups_f64.py with the bound it derives, evaluated one step at a time from
the float32 state and the gradient the device step read.

64 x 64 frames, 2 clips, 2 in / 2 out, hidden 8, two layers, one conv layer: ChebConv, GCNConv, TransformerConv and
MHTransformerConv.  The first and the third train on the flat vector under FlatAdam (plain tensor ops on the flat buffer), the
other two on a parameter list under torch's fused Adam (torch._foreach_* on sub-lists).  The setting is the README's mixed example
with one zero-scale pair in front of it, so that every kind of entry occurs: unit, scaled and decayed, decayed only, kept."""
import copy
import functools
import random

import numpy as np
import pytest
import torch

import ema_restated
import groups_f64
from groups_f64 import ALL_UNIT
from helpers import dev

pytestmark = pytest.mark.gpu

T_IN, T_OUT, NORM = 2, 2, 0.05          # (a clipping norm far below the gradients' so that the global norm takes part)
CONVS = ['ChebConv', 'GCNConv', 'TransformerConv', 'MHTransformerConv']
FLAT = ('ChebConv', 'TransformerConv')
MIXED = [('decoder.fc_out1.*', dict(lr_scale=0.0, weight_decay=1e-2))] + groups_f64.MIXED
MASK = np.zeros((64, 64), dtype=bool)
MASK[:, 58:] = True


@pytest.fixture(autouse=True)
def _quiet(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)             # (initiate_training()'s SummaryWriter writes under the working directory)


@functools.lru_cache(maxsize=None)
def _clips():
    """Eight clips (x (8, T_IN, 64, 64, 1), y (8, T_OUT, 64, 64, 1)) on the device, made once, not modified."""
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(7, 0, 8, T_IN, T_OUT, n_digits=1, pixel_noise=0.02)
    return torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())


def _batch(i):
    x, y = _clips()
    return x[2 * (i % 4):2 * (i % 4) + 2], y[2 * (i % 4):2 * (i % 4) + 2]


def _pair(conv, capturable=False, static=False, train_mode=True, n=2):
    """n predictors with the same weights: one is made, the others are deep copies; each then gets its own optimiser."""
    from model.mpnnlstm import NextFramePredictorS2S
    torch.manual_seed(5)
    first = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T_IN, output_timesteps=T_OUT, device=dev(),
                                  model_kwargs=dict(hidden_size=8, dropout=0.1, n_layers=2, n_conv_layers=1, convolution_type=conv))
    with torch.no_grad():
        for p in first.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    first.model.train(train_mode)
    made = [first] + [copy.deepcopy(first) for _ in range(n - 1)]
    for nfp in made:
        nfp.initiate_training(lr=0.01, lr_decay=0.5, capturable=capturable)
        nfp.model.static_shapes = static
    assert all((nfp.flat is not None) == (conv in FLAT) for nfp in made)
    return made


def _seeded(run):
    """run() from fixed seeds of everything a step draws from."""
    from qtmpnn import ops
    torch.manual_seed(11)
    random.seed(3)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())
    return run()


def _adam(nfp):
    """{'exp_avg' / 'exp_avg_sq': {name: host tensor}, 'step': int} of either optimiser (zeros where there is no state yet)."""
    from qtmpnn.optim import adam_state
    if nfp.flat is not None:
        return adam_state(nfp.optimizer, nfp.model)
    out, steps = {'exp_avg': {}, 'exp_avg_sq': {}}, [0]
    for k, p in nfp.model.named_parameters():
        st = nfp.optimizer.state.get(p)
        for key in out:
            out[key][k] = st[key].detach().cpu().clone() if st else torch.zeros(p.shape)
        if st:
            steps.append(int(float(st['step'])))
    return dict(out, step=max(steps))


def _params(nfp):
    return {k: p.detach().clone() for k, p in nfp.model.named_parameters()}


def _same_training_state(a, b):
    """Parameters and both Adam moments, by name, bit for bit."""
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k
    sa, sb = _adam(a), _adam(b)
    assert sa['step'] == sb['step']
    for key in ('exp_avg', 'exp_avg_sq'):
        for k in sa[key]:
            assert torch.equal(sa[key][k], sb[key][k]), (key, k)


def _step(nfp, i):
    return nfp.train_step(*_batch(i), None, MASK, max_norm=NORM)


def _flat(named):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in named.values()])


def _vectors(nfp):
    """(s, lam) per entry of the flat parameter vector, from the predictor's table."""
    table = nfp.param_group_table
    sizes = [p.numel() for p in nfp.model.parameters()]
    return tuple(np.repeat([table[n][k] for n in table], sizes) for k in (0, 1))


# -- (a) no setting is a no-op -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_plain_steps_on_deep_copies_give_equal_bits(conv):
    """The ground the other cases stand on (it holds without the feature as well): two copies, the same seeds, the same bits."""
    a, twin = _pair(conv)
    la = _seeded(lambda: [_step(a, i) for i in range(2)])
    lt = _seeded(lambda: [_step(twin, i) for i in range(2)])
    assert all(torch.equal(x, y) and bool(torch.isfinite(x)) for x, y in zip(la, lt))
    _same_training_state(a, twin)


@pytest.mark.parametrize('conv', CONVS)
def test_none_and_an_all_unit_setting_are_the_plain_step(conv):
    none, unit, twin = _pair(conv, n=3)
    none.set_param_groups(None)
    unit.set_param_groups(ALL_UNIT)
    assert unit.param_group_table == twin.param_group_table and set(unit.param_group_table.values()) == {(1.0, 0.0)}
    losses = [_seeded(lambda nfp=nfp: [_step(nfp, i) for i in range(2)]) for nfp in (none, unit, twin)]
    for got in losses[:2]:
        assert all(torch.equal(x, y) for x, y in zip(got, losses[2]))
    _same_training_state(none, twin)
    _same_training_state(unit, twin)


# -- (b) the mixed setting: the twin's bits where they must be, the float64 model everywhere ---------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_mixed_setting_keeps_unit_and_zero_scale_bits_and_the_float64_bound(conv):
    """Worst |device - model| / bound over the three steps on an MI355X (profiles/groups.txt has the run): parameters 0.30
    (ChebConv), 0.31 (GCNConv), 0.48 (TransformerConv), 0.49 (MHTransformerConv); moments at most 0.25."""
    a, twin = _pair(conv)
    a.set_param_groups(MIXED)
    s, lam = _vectors(a)
    unit, kept = (s == 1) & (lam == 0), s == 0
    assert unit.any() and kept.any() and ((s == 1) & (lam > 0)).any() and ((s != 1) & (s != 0) & (lam > 0)).any()
    form = 'flat' if conv in FLAT else 'list'
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0}
    for t in range(1, 4):
        before, state = _flat(_params(a)), _adam(a)
        m, v = _flat(state['exp_avg']), _flat(state['exp_avg_sq'])
        lr = float(a.optimizer.param_groups[0]['lr'])

        def run(nfp):
            nfp.zero_grad()
            loss = nfp.forward_loss(*_batch(t), None, MASK)
            loss.backward()
            clip = nfp._grads_ready()
            g = nfp._grad_flat().detach().cpu().numpy().copy()
            nfp._clip_and_step(clip, NORM)
            return loss.detach(), g
        (loss, g) = _seeded(lambda: run(a))
        assert np.sqrt((g.astype(np.float64) ** 2).sum()) > NORM, 'the clipping does not act: the global norm is not compared'
        after, state = _flat(_params(a)), _adam(a)
        got = dict(p=after, m=_flat(state['exp_avg']), v=_flat(state['exp_avg_sq']))
        assert state['step'] == t
        out = groups_f64.grouped_step(before, g, m, v, t, s, lam, lr=lr, max_norm=NORM, form=form)
        bound = groups_f64.grouped_bound(before, g, m, v, t, out)
        w = groups_f64.worst(got, out, bound)
        print(f'{conv} step {t} (lr {lr}): worst |device - model| / bound {w}')
        worst = {k: max(worst[k], w[k]) for k in worst}
        assert np.array_equal(after[kept], before[kept]), 'zero scale keeps the parameter bits'
        assert got['m'][kept].any() and got['v'][kept].any(), 'and its moments advance'
        if t == 1:
            (tl, tg) = _seeded(lambda: run(twin))
            assert torch.equal(loss, tl) and np.array_equal(g, tg)
            plain = _flat(_params(twin))
            assert np.array_equal(after[unit], plain[unit]), 'unit entries have the plain step\'s bits'
            moved = ~unit & ~kept
            assert (after[moved] != plain[moved]).mean() > 0.5, 'the other entries take another step'
            ts = _adam(twin)
            assert np.array_equal(got['m'], _flat(ts['exp_avg'])) and np.array_equal(got['v'], _flat(ts['exp_avg_sq'])), \
                'the moments are the plain step\'s, for every entry'
        for _ in range(3 if t == 2 else 0):
            a.scheduler.step()              # (StepLR with step_size 3: the third step runs at half the learning rate)
    assert float(a.optimizer.param_groups[0]['lr']) == 0.005
    print(f'RATIO {conv} {worst["p"]:.4f} {worst["m"]:.4f} {worst["v"]:.4f}')
    assert all(r <= 1.0 for r in worst.values()), worst


# -- (c) eager = captured ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_eager_and_captured_steps_give_equal_bits(conv):
    eager, graphed = _pair(conv, capturable=True, static=True, train_mode=False)
    for nfp in (eager, graphed):
        nfp.set_param_groups(MIXED)
    start = _params(eager)
    step = graphed.make_graphed_step(*_batch(0), None, MASK, warmup=1, max_norm=NORM)       # (the warm-up is a real step)
    assert step.param_groups == graphed._groups and step.param_groups is not None
    _step(eager, 0)
    for i in (1, 2):
        le, lg = _step(eager, i), step(*_batch(i))
        assert torch.equal(le, lg), (i, le, lg)
        for nfp in (eager, graphed):
            for _ in range(3 if i == 1 else 0):
                nfp.scheduler.step()        # (the learning rate is a device tensor: the replay follows it)
    _same_training_state(graphed, eager)
    s, _ = _vectors(eager)
    now, was = _flat(_params(eager)), _flat(start)
    assert np.array_equal(now[s == 0], was[s == 0]) and (now[s != 0] != was[s != 0]).mean() > 0.5
    step.check()


# -- (d) frozen entries are left alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_frozen_entries_get_neither_decay_nor_update(conv):
    (a,) = _pair(conv, n=1)
    a.set_param_groups([('*', dict(weight_decay=1e-2))])
    a.set_trainable(('decoder.*',))
    start = _params(a)
    for i in range(2):
        _step(a, i)
    state = _adam(a)
    for k, p in a.model.named_parameters():
        if k.startswith('encoder.'):
            assert torch.equal(p, start[k]), f'{k} is frozen and moved'
            assert not bool(state['exp_avg'][k].any()) and not bool(state['exp_avg_sq'][k].any()), k
        else:
            assert not torch.equal(p, start[k]), k


# -- (e) the average follows the grouped step --------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_the_average_is_that_of_the_grouped_iterates(conv):
    (a,) = _pair(conv, n=1)
    a.set_param_groups(MIXED)
    a.set_ema(0.9)
    iterates = []
    for i in range(3):
        _step(a, i)
        iterates.append(_flat(_params(a)))
    ref = ema_restated.model64(iterates, 0.9)[-1]
    shadow = _flat(a.ema.state(a.model)['shadow'])
    assert ema_restated.holds(shadow, None, ref), ema_restated.worst(shadow, None, ref)
    stale = ema_restated.model64([iterates[0]] * 3, 0.9)[-1]
    assert not ema_restated.holds(shadow, None, stale), 'the check tells the iterates apart'


# -- (f) resume --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_a_resumed_run_under_the_same_setting_ends_in_the_same_bits(conv, tmp_path):
    whole, first, resumed = _pair(conv, n=3, train_mode=False)
    for nfp in (whole, first):
        nfp.set_param_groups(MIXED)
    for i in range(4):
        _step(whole, i)
    for i in range(2):
        _step(first, i)
    first.save_checkpoint(tmp_path / 'c.pt')
    resumed.load_checkpoint(tmp_path / 'c.pt')
    assert resumed._groups is None, 'the setting is no training state'
    resumed.set_param_groups(MIXED)
    for i in (2, 3):
        _step(resumed, i)
    _same_training_state(resumed, whole)
    ckpt = torch.load(tmp_path / 'c.pt', weights_only=True)
    assert ckpt['format'] == 1 and not any('group' in str(k) for k in ckpt)


# -- (g) a captured step keeps its setting; captured accumulation ------------------------------------------------------------------
@pytest.mark.parametrize('conv', CONVS)
def test_a_captured_step_is_refused_under_another_setting_and_accumulation_matches_eager(conv):
    eager, graphed = _pair(conv, capturable=True, static=True, train_mode=False)
    for nfp in (eager, graphed):
        nfp.set_param_groups(MIXED)
    group = [_batch(0), _batch(1)]
    step = graphed.make_graphed_step(*group[0], None, MASK, warmup=1, max_norm=NORM, accumulate=2)
    eager.accumulated_step([group[0]], MASK, max_norm=NORM)
    assert torch.equal(eager.accumulated_step(group, MASK, max_norm=NORM), step(group))
    _same_training_state(graphed, eager)
    before = _params(graphed)
    for other in (None, [('decoder.*', dict(lr_scale=0.5))]):
        graphed.set_param_groups(other)
        with pytest.raises(RuntimeError, match=r"^param_groups: this step was captured under param_groups=\[\('decoder\.fc_out1"):
            step(group)
    assert all(torch.equal(p, before[k]) for k, p in graphed.model.named_parameters()), 'a refused replay changes nothing'
    graphed.set_param_groups(MIXED)         # the setting it was captured under again: it runs
    assert bool(torch.isfinite(step(group)))
    step.check()
