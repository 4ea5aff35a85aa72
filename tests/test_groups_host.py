"""Parameter groups on the host (set_param_groups, train(param_groups=), param_group_table): the pure resolution and every refusal
by message, the float64 model of tests/groups_f64.py against torch.optim.AdamW with real parameter groups, the float32 emulation
of the mechanism against the model's own bound with two tampered forms that must miss it, and the parameter-list form of the
mechanism on a predictor without a device."""
import copy
import inspect
import os

import numpy as np
import pytest
import torch

import groups_f64
import pack_f64
from groups_f64 import ALL_UNIT, MIXED
from helpers import ROOT, TinyLoader
from qtmpnn.groups import GroupedStep, as_pairs, check_groups, resolve_groups

NAMES = ['encoder.rnns.0.b_i', 'encoder.rnns.0.w.weight', 'encoder.norm_h.weight', 'decoder.rnns.0.b_i', 'decoder.fc_out1.lins.0.weight',
         'decoder.fc_out2.bias', 'decoder.norm_o.weight']
T_ = 2


# -- the pure parts ---------------------------------------------------------------------------------------------------------------
def test_the_first_matching_pair_decides_and_the_rest_has_the_defaults():
    unit = {n: (1.0, 0.0) for n in NAMES}
    assert resolve_groups(NAMES, None) == unit and list(resolve_groups(NAMES, None)) == NAMES
    got = resolve_groups(NAMES, [('*norm*', {}), ('*bias*', {}), ('encoder.*', dict(lr_scale=0.1, weight_decay=1e-2)),
                                 ('*', dict(weight_decay=1e-2))])
    assert got == {'encoder.rnns.0.b_i': (0.1, 0.01), 'encoder.rnns.0.w.weight': (0.1, 0.01), 'encoder.norm_h.weight': (1.0, 0.0),
                   'decoder.rnns.0.b_i': (1.0, 0.01), 'decoder.fc_out1.lins.0.weight': (1.0, 0.01), 'decoder.fc_out2.bias': (1.0, 0.0),
                   'decoder.norm_o.weight': (1.0, 0.0)}
    assert list(got) == NAMES
    # the order of the pairs decides, not that of the names; a dict is read in its insertion order
    assert resolve_groups(NAMES, {'decoder.fc_out*': dict(lr_scale=2), 'decoder.*': dict(lr_scale=0)})['decoder.fc_out2.bias'] == (2.0, 0.0)
    assert resolve_groups(NAMES, {'decoder.fc_out*': dict(lr_scale=2), 'decoder.*': dict(lr_scale=0)})['decoder.rnns.0.b_i'] == (0.0, 0.0)
    # a name that nothing matches keeps (1, 0)
    assert resolve_groups(NAMES, [('decoder.*', dict(weight_decay=0.5))])['encoder.rnns.0.b_i'] == (1.0, 0.0)
    assert resolve_groups(NAMES, [('*.b_i', dict(lr_scale=np.float32(0.5), weight_decay=3))])['decoder.rnns.0.b_i'] == (0.5, 3.0)
    assert check_groups(None) is None and as_pairs(None) is None
    setting = check_groups([('a', {}), ('b', dict(weight_decay=1))])
    assert setting == (('a', (1.0, 0.0)), ('b', (1.0, 1.0))) and check_groups(as_pairs(setting)) == setting


inf, nan = float('inf'), float('nan')
BAD = [('decoder.*', TypeError, 'plain string'), (b'decoder.*', TypeError, 'plain string'), ((), ValueError, 'empty'),
       ([], ValueError, 'empty'), ({}, ValueError, 'empty'), (7, TypeError, 'sequence'), ({'decoder.*'}, TypeError, 'sequence'),
       (['decoder.*'], TypeError, r'pair \(pattern: str, options: dict\)'), ([('decoder.*',)], TypeError, 'pair'),
       ([('decoder.*', 0.1)], TypeError, 'pair'), ([(3, {})], TypeError, 'pair'), ([('decoder.*', {}, {})], TypeError, 'pair'),
       ([('decoder.*', dict(lr=0.1))], ValueError, r"unknown option 'lr' of the pattern 'decoder\.\*'.*'lr_scale', 'weight_decay'"),
       ([('decoder.*', dict(lr_scale=True))], TypeError, 'lr_scale .*finite number >= 0, got True'),
       ([('decoder.*', dict(lr_scale='1'))], TypeError, 'lr_scale'), ([('decoder.*', dict(lr_scale=None))], TypeError, 'lr_scale'),
       ([('decoder.*', dict(lr_scale=-0.1))], ValueError, 'lr_scale .*>= 0, got -0.1'),
       ([('decoder.*', dict(lr_scale=inf))], ValueError, 'lr_scale'), ([('decoder.*', dict(lr_scale=nan))], ValueError, 'lr_scale'),
       ([('decoder.*', dict(weight_decay=False))], TypeError, 'weight_decay .*finite number >= 0, got False'),
       ([('decoder.*', dict(weight_decay=-1))], ValueError, 'weight_decay'), ([('decoder.*', dict(weight_decay=inf))], ValueError, 'weight_decay'),
       ([('decoder.*', dict(weight_decay=nan))], ValueError, 'weight_decay'), ([('decoder.*', dict(weight_decay=[1]))], TypeError, 'weight_decay'),
       ([('decode.*', {})], ValueError, r"'decode\.\*' is the first match of no parameter: it matches no name.*'encoder', 'decoder'"),
       ([('*', {}), ('decoder.*', dict(lr_scale=0.1))], ValueError,
        r"'decoder\.\*' is the first match of no parameter: it is shadowed.*earlier pattern \('\*',\).*'encoder', 'decoder'"),
       ([('decoder.fc*', {}), ('decoder.r*', {}), ('decoder.[fr]*', {})], ValueError, r"shadowed.*\('decoder\.r\*', 'decoder\.fc\*'\)")]


@pytest.mark.parametrize('bad,error,match', BAD, ids=[repr(b) for b, _, _ in BAD])
def test_resolve_refuses_by_name(bad, error, match):
    with pytest.raises(error, match='^param_groups: .*' + match):
        resolve_groups(NAMES, bad)


# -- the float64 model is torch's AdamW with real parameter groups -----------------------------------------------------------------
def test_the_float64_model_is_torchs_adamw_with_real_groups():
    rng = np.random.default_rng(2)
    settings = [(1.0, 0.0), (0.1, 1e-2), (1.0, 1e-2), (0.0, 0.3), (2.5, 0.0)]
    n, lr0, gamma, norm = 37, 0.01, 0.5, 0.7
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n))) for _ in settings]
    # ONE learning rate and its StepLR, as the project's optimiser holds them; the groups scale it
    opt = torch.optim.AdamW([dict(params=[p], lr=lr0 * s, weight_decay=lam) for p, (s, lam) in zip(params, settings)], lr=lr0)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=gamma)
    p = np.concatenate([q.detach().numpy() for q in params])
    s = np.repeat([a for a, _ in settings], n)
    lam = np.repeat([b for _, b in settings], n)
    m, v, lr = np.zeros_like(p), np.zeros_like(p), lr0
    for t in range(1, 6):
        g = rng.standard_normal(p.size) * (1.0 if t % 2 else 0.01)          # (clipped and unclipped steps)
        for q, gq in zip(params, np.split(g, len(params))):
            q.grad = torch.from_numpy(gq.copy())
        torch.nn.utils.clip_grad_norm_(params, max_norm=norm)
        opt.step()
        sched.step()
        out = groups_f64.grouped_step(p, g, m, v, t, s, lam, lr=lr, max_norm=norm, exact=True)
        p, m, v = out['p'], out['m'], out['v']
        lr = lr0 * gamma ** (t // 3)
        want = np.concatenate([q.detach().numpy() for q in params])
        assert np.max(np.abs(p - want) / np.abs(want)) <= 1e-12, t
        for key, mine in (('exp_avg', m), ('exp_avg_sq', v)):
            theirs = np.concatenate([opt.state[q][key].numpy() for q in params])
            assert np.max(np.abs(mine - theirs)) <= 1e-12 * np.max(np.abs(theirs)), (t, key)
    assert lr == lr0 * gamma and opt.param_groups[1]['lr'] == pytest.approx(lr0 * gamma * 0.1, rel=1e-15), 'the StepLR change was in it'
    assert np.array_equal(p[3 * n:4 * n], np.concatenate([q.detach().numpy() for q in params])[3 * n:4 * n])


# -- the float32 emulation of the mechanism keeps the bound; tampered forms miss it ------------------------------------------------
def _case(seed, n=4097, kind='clipped'):
    rng = np.random.default_rng(seed)
    p = (0.3 * rng.standard_normal(n)).astype(np.float32)
    g = pack_f64.adam_gradient(rng, kind, n)
    m = (0.01 * rng.standard_normal(n)).astype(np.float32)
    v = (1e-4 * rng.random(n)).astype(np.float32)
    s = rng.choice(np.float32([1.0, 0.1, 0.0, 2.5, 1.0]), n)
    lam = rng.choice(np.float32([0.0, 1e-2, 0.3]), n)
    return p, g, m, v, s, lam


@pytest.mark.parametrize('t', [1, 10, 1000])
@pytest.mark.parametrize('kind', ['clipped', 'unclipped'])
def test_the_float32_mechanism_keeps_the_bound_and_the_tampered_forms_miss_it(kind, t):
    p, g, m, v, s, lam = _case(7 + t, kind=kind)
    out = groups_f64.grouped_step(p, g, m, v, t, s, lam)
    bound = groups_f64.grouped_bound(p, g, m, v, t, out)
    got = groups_f64.emulate_grouped(p, g, m, v, t, s, lam)
    w = groups_f64.worst(got, out, bound)
    print(f'{kind} t={t}: worst |emulation - model| / bound {w}')
    assert all(r <= 1.0 for r in w.values()), w
    unit, kept = (s == 1) & (lam == 0), s == 0
    plain = pack_f64.emulate_adam(p, g, m, v, t)
    assert unit.any() and np.array_equal(got['p'][unit], plain['p'][unit]), 'unit entries have the plain step\'s bits'
    assert kept.any() and np.array_equal(got['p'][kept], p[kept]), 'zero scale keeps the bits (its decay factor is exactly 1)'
    assert np.array_equal(got['m'], plain['m']) and np.array_equal(got['v'], plain['v']) and bool(got['m'][kept].any())
    for tamper in groups_f64.TAMPERS:
        bad = groups_f64.worst(groups_f64.emulate_grouped(p, g, m, v, t, s, lam, tamper=tamper), out, bound)
        print(f'{kind} t={t}: {tamper}: {bad}')
        assert bad['p'] > 1.0, (tamper, bad)


def test_the_bound_is_the_plain_adam_bound_on_unit_entries_and_states_its_multiples():
    p, g, m, v, s, lam = _case(3)
    out = groups_f64.grouped_step(p, g, m, v, 5, s, lam)
    bound = groups_f64.grouped_bound(p, g, m, v, 5, out)
    plain = pack_f64.adam_step(p, g, m, v, 5)
    unit = (s == 1) & (lam == 0)
    assert np.array_equal(bound['p'][unit], pack_f64.adam_bound(p, g, m, v, 5, plain)['p'][unit])
    assert np.array_equal(out['p'][unit], plain['p'][unit])
    # the blend's share stays below (4 s + 1) ulp(|p|), the decay's below 2 + 3 lr s lam, doubled, beyond the (scaled) Adam bound
    P = np.maximum(np.abs(out['p1']), np.maximum(np.abs(out['q']), np.abs(out['p'])))
    extra = bound['p'] - 2.0 * np.where(s != 1, s, 1.0) * (pack_f64.adam_bound(out['p1'], g, m, v, 5, out)['p'] / 2.0)
    allowed = 2.0 * pack_f64.U * (np.where(s != 1, 4.0 * s + 1.0, 0.0) * P * (1 + 1e-6) + np.where(s * lam != 0, 3.0, 0.0) * np.abs(p))
    assert np.all(extra <= allowed + 1e-30)


# -- the mechanism's vectors -------------------------------------------------------------------------------------------------------
def test_the_vectors_follow_the_table_and_the_trainable_flags():
    table = [('a', 0, (2, 3)), ('b', 6, (4,)), ('c', 10, ()), ('d', 11, (1, 2))]
    params = [torch.zeros(shape) for _, _, shape in table]
    gs = GroupedStep(params, table)
    gs.set({'a': (1.0, 0.0), 'b': (0.1, 0.5), 'c': (0.0, 2.0), 'd': (1.0, 0.25)})
    f = np.float32
    assert gs.s.tolist() == [1.0] * 6 + [float(f(0.1))] * 4 + [0.0] + [1.0] * 2
    assert gs.nsl.tolist() == [0.0] * 6 + [-float(f(f(0.1) * f(0.5)))] * 4 + [0.0] + [-0.25] * 2
    assert gs.blended.tolist() == [False] * 6 + [True] * 5 + [False] * 2 and gs.decay and gs.blend
    assert [len(l) for l in gs._decay_lists] == [2, 2] and [len(l) for l in gs._blend_lists] == [2, 2, 2, 2]
    held = (gs.s.data_ptr(), gs.nsl.data_ptr(), gs.work.data_ptr(), gs.stash.data_ptr(), gs.blended.data_ptr())
    gs.set({'a': (1.0, 0.0), 'b': (0.1, 0.5), 'c': (0.0, 2.0), 'd': (1.0, 0.25)}, (True, False, True, False))
    assert not gs.decay and gs.blend and not bool(gs.nsl.any()) and gs.blended.tolist() == [False] * 10 + [True] + [False] * 2
    gs.set({k: (1.0, 0.0) for k in 'abcd'})
    assert not gs.decay and not gs.blend
    assert held == (gs.s.data_ptr(), gs.nsl.data_ptr(), gs.work.data_ptr(), gs.stash.data_ptr(), gs.blended.data_ptr()), 'filled in place'


@pytest.mark.parametrize('flat', [True, False])
def test_the_launches_are_the_emulation_bit_for_bit(flat):
    """GroupedStep's two halves around a stand-in step (p -= a fixed update) against the same statements in numpy float32."""
    rng = np.random.default_rng(5)
    table, off = [], 0
    for k, shape in enumerate([(3, 5), (7,), (), (2, 2), (9,)]):
        table.append((f'p{k}', off, shape))
        off += int(np.prod(shape, dtype=int))
    resolved = {'p0': (1.0, 0.0), 'p1': (0.1, 1e-2), 'p2': (0.0, 0.5), 'p3': (2.5, 0.0), 'p4': (1.0, 0.3)}
    vec = torch.from_numpy((0.3 * rng.standard_normal(off)).astype(np.float32))
    upd = torch.from_numpy((0.01 * rng.standard_normal(off)).astype(np.float32))
    start = vec.clone()
    views = [vec[o:o + int(np.prod(sh, dtype=int))].view(sh) for _, o, sh in table]
    gs = GroupedStep(vec if flat else views, table)
    gs.set(resolved)
    for lr in (0.01, torch.tensor(0.005)):
        before = vec.clone().numpy()
        gs.before(lr)
        vec.sub_(upd)
        gs.after()
        f, lr32 = np.float32, np.float32(float(lr))
        s, nsl = gs.s.numpy(), gs.nsl.numpy()
        p0 = before * (f(1) + nsl * lr32)
        q = p0 - upd.numpy()
        want = np.where(s != 1, (q - p0) * s + p0, q)
        assert np.array_equal(vec.numpy(), want)
        assert np.array_equal(vec.numpy()[15:22] != before[15:22], np.ones(7, bool))
        assert vec.numpy()[22] == before[22], 's = 0 keeps the bits'
        assert np.array_equal(vec.numpy()[:15], (before - upd.numpy())[:15]), 'unit entries: the plain step'
    assert not torch.equal(vec, start)


# -- the predictor ----------------------------------------------------------------------------------------------------------------
def _predictor(monkeypatch, tmp_path, **kwargs):
    """A predictor without a device that records what would run (tests/test_trainable_host.py's)."""
    from model.mpnnlstm import NextFramePredictorS2S
    from model.seq2seq import Seq2Seq
    from qtmpnn import _lib
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1), **kwargs)
    nfp.ran = []
    record = lambda what: lambda *a, **k: nfp.ran.append(what)
    monkeypatch.setattr(nfp, 'train_step', record('train_step'))
    monkeypatch.setattr(nfp, '_inference', record('_inference'))
    monkeypatch.setattr(Seq2Seq, 'forward', record('forward'))
    monkeypatch.setattr(_lib, 'call', record('call'))
    monkeypatch.setattr(_lib, 'load', record('load'))
    return nfp


@pytest.fixture
def cpu_predictor(monkeypatch, tmp_path):
    return _predictor(monkeypatch, tmp_path)


def _loader(n=2):
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    return TinyLoader([(x[None], y[None], torch.zeros(1))] * n, (64, 64))


def _state(nfp):
    return nfp._groups, nfp._grouped, [p.detach().clone() for p in nfp.model.parameters()]


def _same_state(a, b):
    return a[0] == b[0] and a[1] is b[1] and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


@pytest.mark.parametrize('bad,error,match', BAD[:8] + BAD[12:14] + BAD[16:17] + BAD[-3:-1], ids=repr)
def test_a_bad_setting_is_refused_by_name_before_anything_runs(cpu_predictor, bad, error, match):
    nfp = cpu_predictor
    with pytest.raises(error, match='^param_groups: '):
        nfp.train(_loader(), _loader(), n_epochs=1, param_groups=bad)
    assert nfp.ran == [] and not nfp.training_initiated
    with pytest.raises(error, match='^param_groups: '):
        nfp.set_param_groups(bad)                   # (before the complaint about the missing optimiser)
    nfp.initiate_training(0.01, 0.5)
    nfp.set_param_groups(MIXED)
    before = _state(nfp)
    for refused in (lambda: nfp.set_param_groups(bad), lambda: nfp.train(_loader(), _loader(), n_epochs=1, param_groups=bad)):
        with pytest.raises(error, match='^param_groups: '):
            refused()
    assert _same_state(before, _state(nfp)) and nfp.ran == []


def test_the_setting_follows_the_optimiser_and_the_table_lists_it(cpu_predictor):
    nfp = cpu_predictor
    names = [n for n, _ in nfp.model.named_parameters()]
    assert nfp.param_group_table == {n: (1.0, 0.0) for n in names}
    nfp.set_param_groups(None)                      # no setting on what has none needs no optimiser
    with pytest.raises(ValueError, match='^param_groups: .*initiate_training'):
        nfp.set_param_groups(MIXED)
    assert not nfp.training_initiated and nfp.ran == [] and nfp._grouped is None
    nfp.initiate_training(0.01, 0.5)
    nfp.set_param_groups(MIXED)
    table = nfp.param_group_table
    assert list(table) == names and set(table.values()) == {(1.0, 0.0), (0.1, 0.01), (1.0, 0.01)}
    for n, (s, lam) in table.items():
        plain = 'norm' in n or 'bias' in n
        assert (s, lam) == ((1.0, 0.0) if plain else (0.1, 0.01) if n.startswith('encoder.') else (1.0, 0.01)), n
    assert len(nfp.optimizer.param_groups) == 1, 'the optimiser keeps ONE group'
    held = nfp._grouped
    nfp.set_param_groups(dict(MIXED))
    assert nfp._grouped is held, 'the vectors are made once per optimiser'
    nfp.initiate_training(0.01, 0.5)
    assert nfp._groups is None and nfp._grouped is None and nfp.param_group_table == {n: (1.0, 0.0) for n in names}
    assert nfp.ran == []


def _stepper(nfps):
    """One optimiser step on every predictor of `nfps` with the same fixed random gradients, through _clip_and_step."""
    g = torch.Generator().manual_seed(4)

    def step(max_norm=1.0):
        grads = [torch.randn(p.shape, generator=g) for p in nfps[0].model.parameters()]
        for nfp in nfps:
            for p, gr in zip(nfp.model.parameters(), grads):
                p.grad = gr.clone() if p.requires_grad else None
            nfp._clip_and_step(nfp._grads_ready(), max_norm)
        return grads
    return step


def _moments(nfp):
    return [(nfp.optimizer.state[p]['exp_avg'], nfp.optimizer.state[p]['exp_avg_sq']) if nfp.optimizer.state.get(p) else None
            for p in nfp.model.parameters()]


def test_no_setting_and_an_all_unit_setting_are_the_plain_step(cpu_predictor):
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    twin, unit = copy.deepcopy(nfp), copy.deepcopy(nfp)
    nfp.set_param_groups(None)
    unit.set_param_groups(ALL_UNIT)
    assert unit._grouped is not None and not unit._grouped.decay and not unit._grouped.blend
    step = _stepper([nfp, twin, unit])
    for _ in range(3):
        step()
    for other in (twin, unit):
        assert all(torch.equal(p, q) for p, q in zip(nfp.model.parameters(), other.model.parameters()))
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(_moments(nfp), _moments(other)))


def test_the_parameter_list_step_is_the_float64_model_and_keeps_what_it_must(cpu_predictor):
    """Three steps with one StepLR change on the CPU predictor (torch's Adam over the parameter list) against the float64 model,
    within its bound; unit entries equal a plain twin after ONE step, zero-scale entries keep their bits while their moments
    move, frozen entries get neither decay nor update, and the average follows the blend."""
    import ema_restated
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    twin = copy.deepcopy(nfp)
    setting = [('*norm*', {}), ('*bias*', {}), ('decoder.fc_out*', dict(lr_scale=0.0, weight_decay=0.0)),
               ('encoder.*', dict(lr_scale=0.1, weight_decay=1e-2)), ('*', dict(weight_decay=1e-2))]
    nfp.set_param_groups(setting)
    nfp.set_ema(0.9)
    table = nfp.param_group_table
    names = list(table)
    sizes = [p.numel() for p in nfp.model.parameters()]
    s, lam = (np.repeat([table[n][k] for n in names], sizes) for k in (0, 1))
    flat = lambda tensors: np.concatenate([t.detach().numpy().reshape(-1) for t in tensors])
    step, plain_step = _stepper([nfp]), _stepper([twin])
    m = v = np.zeros(sum(sizes), np.float32)
    iterates = []
    for t in range(1, 4):
        p0 = flat(nfp.model.parameters())
        lr = nfp.optimizer.param_groups[0]['lr']
        g = flat(step(max_norm=1.0))
        out = groups_f64.grouped_step(p0, g, m, v, t, s, lam, lr=lr, max_norm=1.0, form='list')
        bound = groups_f64.grouped_bound(p0, g, m, v, t, out)
        got = dict(p=flat(nfp.model.parameters()), m=flat(a for a, _ in _moments(nfp)), v=flat(b for _, b in _moments(nfp)))
        w = groups_f64.worst(got, out, bound)
        print(f'step {t} (lr {lr}): worst |step - model| / bound {w}')
        assert all(r <= 1.0 for r in w.values()), (t, w)
        if t == 1:
            plain_step(max_norm=1.0)
            unit = (s == 1) & (lam == 0)
            assert unit.any() and np.array_equal(got['p'][unit], flat(twin.model.parameters())[unit])
            assert not np.array_equal(got['p'][~unit & (s != 0)], flat(twin.model.parameters())[~unit & (s != 0)])
        assert (s == 0).any() and np.array_equal(got['p'][s == 0], p0[s == 0]) and got['m'][s == 0].any()
        m, v = got['m'], got['v']
        iterates.append(got['p'])
        for _ in range(3 if t == 2 else 0):
            nfp.scheduler.step()
    assert nfp.optimizer.param_groups[0]['lr'] == 0.005
    ref = ema_restated.model64(iterates, 0.9)[-1]
    assert ema_restated.holds(flat(nfp.ema.shadow), None, ref), 'the shadow averages what the grouped step wrote'
    # frozen entries: neither decay nor update
    nfp.set_trainable(('decoder.*',))
    held = {k: p.detach().clone() for k, p in nfp.model.named_parameters()}
    step(max_norm=1.0)
    for k, p in nfp.model.named_parameters():
        assert torch.equal(p, held[k]) == (k.startswith('encoder.') or table[k][0] == 0.0), k


def test_inside_averaged_weights_the_setting_is_refused(cpu_predictor):
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    nfp.set_ema(0.9)
    _stepper([nfp])()
    with nfp.averaged_weights():
        before = _state(nfp)
        for refused in (lambda: nfp.set_param_groups(MIXED), lambda: nfp.set_param_groups(None)):
            with pytest.raises(RuntimeError, match=r'^param_groups: set_param_groups\(\) inside averaged_weights'):
                refused()
        assert _same_state(before, _state(nfp))


def test_train_holds_the_setting_for_the_call(cpu_predictor, monkeypatch):
    nfp = cpu_predictor
    seen = []
    monkeypatch.setattr(nfp, 'train_step', lambda *a, **k: seen.append(nfp._groups) or torch.zeros(()))
    monkeypatch.setattr(nfp, '_test_pass', lambda *a, **k: (0.0, 1))
    nfp.train(_loader(), _loader(), n_epochs=1, truncated_backprop=0, param_groups=MIXED)       # (it makes the optimiser, then applies the setting)
    assert seen == [check_groups(MIXED)] * 2 and nfp._groups is None
    other = [('decoder.*', dict(lr_scale=0.5))]
    nfp.set_param_groups(other)
    nfp.train(_loader(), _loader(), n_epochs=1, truncated_backprop=0)                           # left out: the predictor's setting stays
    assert seen[2:] == [check_groups(other)] * 2 and nfp._groups == check_groups(other)
    nfp.train(_loader(1), _loader(), n_epochs=1, truncated_backprop=0, param_groups=None)       # None: no setting, for the call
    assert seen[4:] == [None] and nfp._groups == check_groups(other)

    def fails(*a, **k):
        raise KeyError('inside')
    monkeypatch.setattr(nfp, 'train_step', fails)
    with pytest.raises(KeyError, match='inside'):
        nfp.train(_loader(), _loader(), n_epochs=1, truncated_backprop=0, param_groups=MIXED)
    assert nfp._groups == check_groups(other)


def test_a_captured_step_is_held_to_its_setting(cpu_predictor):
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    nfp.set_param_groups(MIXED)
    held = nfp._groups
    nfp._groups_guard(held)
    for now in (None, [('decoder.*', dict(lr_scale=0.5))]):
        nfp.set_param_groups(now)
        with pytest.raises(RuntimeError, match=r"^param_groups: this step was captured under param_groups=\[\('\*norm\*', "):
            nfp._groups_guard(held)
    nfp.set_param_groups(dict(MIXED))
    nfp._groups_guard(held)
    nfp.set_param_groups(None)
    with pytest.raises(RuntimeError, match='^param_groups: this step was captured under param_groups=None'):
        (nfp.set_param_groups(MIXED), nfp._groups_guard(None))


def test_the_surface_is_what_it_was():
    from model.mpnnlstm import NextFramePredictorS2S as P
    from qtmpnn import _lib
    names = list(inspect.signature(P.train).parameters)
    assert names == ['self', 'loader_train', 'loader_test', 'climatology', 'n_epochs', 'lr', 'lr_decay', 'mask', 'high_interest_region',
                     'truncated_backprop', 'graph_structure', 'use_graph', 'accumulate', 'pos_weight', 'test_graph', 'patience',
                     'min_delta', 'restore_best', 'keep_best', 'monitor', 'loss_weights', 'lead_weights']
    assert list(inspect.signature(P.set_param_groups).parameters) == ['self', 'groups']
    assert isinstance(P.param_group_table, property) and 'param_groups=groups' in P.train.__doc__
    assert len(_lib.exported_names()) == 91
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'set_param_groups' in readme and '(91 entry points)' in readme
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'set_param_groups' in design and 'p0 + s' in design


def test_an_unknown_keyword_is_still_a_type_error(cpu_predictor):
    with pytest.raises(TypeError, match='param_group'):
        cpu_predictor.train(_loader(), _loader(), n_epochs=1, param_group=MIXED)
    assert cpu_predictor.ran == []
