"""Averaged weights, host side (no GPU): WeightEMA on CPU tensors against the float64 model of tests/ema_restated.py, the tampered
float32 forms the checker has to refuse, the state's round trip between the flat and the per-parameter layout, every refusal by
name before anything is launched, and the checkpoint file with and without the average.  The ABI is what it was."""
import inspect

import numpy as np
import pytest
import torch

import ema_restated as R
from helpers import TinyLoader

T_ = 3
NAN = float('nan')
SHAPES = [(5, 7), (11,), ()]                # the list form: three parameters; the flat form: their 47 elements as one vector
DECAYS = [0.0, 0.5, 0.9, 0.999]


def _split(vec):
    out, off = [], 0
    for shape in SHAPES:
        n = int(np.prod(shape, dtype=np.int64))
        out.append(vec[off:off + n].reshape(shape))
        off += n
    return out


def _run(kind, iterates, d):
    """WeightEMA over a CPU parameter that takes the values of `iterates` one after the other -> per update (shadow, averaged),
    as flat float32 arrays."""
    from qtmpnn.ema import WeightEMA
    n = iterates[0].size
    if kind == 'flat':
        params = torch.nn.Parameter(torch.zeros(n))
        write = lambda p: params.data.copy_(torch.from_numpy(p))
        flat = lambda ts: ts.detach().numpy().copy()
        out = torch.empty(n)
    else:
        params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
        write = lambda p: [q.data.copy_(torch.from_numpy(v)) for q, v in zip(params, _split(p))]
        flat = lambda ts: np.concatenate([t.detach().numpy().reshape(-1) for t in ts])
        out = [torch.empty(s) for s in SHAPES]
    ema = WeightEMA(params, d)
    assert ema.updates == 0 and not flat(ema.shadow).any()
    got = []
    for t, p in enumerate(iterates, 1):
        write(p)
        ema.update()
        assert ema.updates == t
        assert ema.averaged(out) is out
        got.append((flat(ema.shadow), flat(out)))
    return got


@pytest.mark.parametrize('kind', ['flat', 'list'])
@pytest.mark.parametrize('d', DECAYS)
def test_updates_keep_the_bound_of_the_float64_model(kind, d):
    """1, 2 and 50 updates (every one of the 50 is looked at) over a moving iterate: shadow and average within the bound."""
    _, iterates = R.walk(5, (47,), 50)
    ref, got = R.model64(iterates, d), _run(kind, iterates, d)
    worst = [R.worst(s, m, r) for (s, m), r in zip(got, ref)]
    print(f'{kind} d={d}: worst error / bound after 1, 2, 50 updates: {worst[0]}, {worst[1]}, {worst[49]}; over all: {np.max(worst):.3f}')
    assert all(R.holds(s, m, r) for (s, m), r in zip(got, ref))
    if d == 0.0:
        assert all(np.array_equal(s, p) and np.array_equal(m, p) for (s, m), p in zip(got, iterates)), 'd = 0 is the last iterate'
    # the bound is no loose one: it is a few ulps of the values
    assert float(np.max(ref[-1]['e_m'] / np.maximum(np.abs(ref[-1]['m']), 1e-3))) < 1e-4


@pytest.mark.parametrize('kind', ['flat', 'list'])
@pytest.mark.parametrize('d', DECAYS)
def test_a_constant_iterate_is_its_own_average_from_the_first_update(kind, d):
    p = R.walk(6, (47,), 1)[0]
    iterates = [p] * 5
    ref, got = R.model64(iterates, d), _run(kind, iterates, d)
    for (s, m), r in zip(got, ref):
        assert np.allclose(r['m'], p.astype(np.float64), rtol=1e-12, atol=0), 'the float64 model itself: the debiased mean of p is p'
        assert np.all(np.abs(m.astype(np.float64) - p) <= r['e_m'])
    if d > 0:
        assert not np.allclose(got[0][0], p, rtol=1e-3), 'the shadow alone starts near zero: that is what the debias is for'


def test_flat_and_list_forms_agree_with_the_float32_yardstick():
    """The yardstick passes the checker it is a yardstick for, and the two forms of WeightEMA stay within the bound of each other's
    model (on the CPU they are the same bits where torch contracts neither or both)."""
    p0, iterates = R.walk(7, (47,), 6)
    for d in DECAYS:
        ref = R.model64(iterates, d)
        clean = R.form32(iterates, d)
        assert all(R.holds(s, m, r) for (s, m), r in zip(clean, ref)), d
        flat, lst = _run('flat', iterates, d), _run('list', iterates, d)
        print(f'd={d}: flat == list bit for bit: {all(np.array_equal(a[1], b[1]) for a, b in zip(flat, lst))}; '
              f'flat == numpy float32 form: {all(np.array_equal(a[1], b[1]) for a, b in zip(flat, clean))}')


@pytest.mark.parametrize('tamper', R.TAMPERS)
def test_the_checker_refuses_every_tampered_form(tamper):
    p0, iterates = R.walk(8, (47,), 6)
    d = 0.9
    ref = R.model64(iterates, d)
    clean, bad = R.form32(iterates, d, p0), R.form32(iterates, d, p0, tamper)
    assert all(R.holds(s, m, r) for (s, m), r in zip(clean, ref))
    failing = [t for t, ((s, m), r) in enumerate(zip(bad, ref), 1) if not R.holds(s, m, r)]
    print(f'{tamper}: fails the checker after updates {failing}; worst error / bound {[R.worst(s, m, r) for (s, m), r in zip(bad, ref)][-1]}')
    assert len(failing) >= 5, 'wrong from the first or second update on, not by a rounding'
    assert not R.holds(*bad[-1], ref[-1])


def test_averaged_before_any_update_is_refused_by_name():
    from qtmpnn.ema import WeightEMA
    ema = WeightEMA(torch.nn.Parameter(torch.ones(4)), 0.9)
    out = torch.full((4,), 7.0)
    with pytest.raises(ValueError, match='^ema: no optimiser step has been averaged yet'):
        ema.averaged(out)
    assert bool((out == 7.0).all())
    for bad, error in ((True, TypeError), ('0.9', TypeError), (None, TypeError), (1.0, ValueError), (-0.1, ValueError), (NAN, ValueError)):
        with pytest.raises(error, match='^ema: '):
            WeightEMA(torch.nn.Parameter(torch.ones(4)), bad)
    with pytest.raises(ValueError, match='^ema: .*fp32'):
        WeightEMA(torch.nn.Parameter(torch.ones(4, dtype=torch.float64)), 0.5)


def test_update_is_in_place_and_allocates_no_tensor_of_its_own():
    """The shadow keeps its storage over updates, averaged() and load_state(): a captured step holds these pointers."""
    from qtmpnn.ema import WeightEMA
    params = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    ema = WeightEMA(params, 0.9)
    ptrs = [s.data_ptr() for s in ema.shadow]
    for _ in range(3):
        ema.update()
    lin = _Named(params)
    st = ema.state(lin)
    ema.load_state(st)
    assert ptrs == [s.data_ptr() for s in ema.shadow] and ema.updates == 3
    assert all(not s.requires_grad for s in ema.shadow)


class _Named(torch.nn.Module):
    """A module whose named_parameters() are a0, a1, a2 over the given tensors, in order."""

    def __init__(self, params):
        super().__init__()
        for i, p in enumerate(params):
            self.register_parameter(f'a{i}', p)


def test_state_round_trip_between_the_flat_and_the_per_parameter_layout():
    from qtmpnn.ema import WeightEMA, check_state
    from qtmpnn.flat import name_table
    _, iterates = R.walk(9, (47,), 4)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    module, vec = _Named(params), torch.nn.Parameter(torch.zeros(47))
    a, b = WeightEMA(params, 0.9), WeightEMA(vec, 0.9)
    for p in iterates:
        vec.data.copy_(torch.from_numpy(p))
        for q, v in zip(params, _split(p)):
            q.data.copy_(torch.from_numpy(v))
        a.update()
        b.update()
    sa, sb = a.state(module), b.state(module)
    table = name_table(module)
    for st in (sa, sb):
        assert set(st) == {'shadow', 'decay', 'updates'} and st['decay'] == 0.9 and type(st['decay']) is float
        assert st['updates'] == 4 and type(st['updates']) is int and list(st['shadow']) == ['a0', 'a1', 'a2']
        assert [tuple(t.shape) for t in st['shadow'].values()] == SHAPES
        check_state(st, table)
    assert sa['shadow']['a0'].data_ptr() != a.shadow[0].data_ptr(), 'copies'
    # either form reads the other's state, in place
    c, d = WeightEMA(params, 0.9), WeightEMA(vec, 0.9)
    ptr = d.shadow.data_ptr()
    c.load_state(sb)
    d.load_state(sa)
    assert c.updates == d.updates == 4 and d.shadow.data_ptr() == ptr
    assert all(torch.equal(x, y) for x, y in zip(c.shadow, b.state(module)['shadow'].values()))
    assert torch.equal(d.shadow, torch.cat([t.reshape(-1) for t in a.shadow]))
    out_c, out_d = [torch.empty(s) for s in SHAPES], torch.empty(47)
    c.averaged(out_c)
    d.averaged(out_d)
    assert np.all(np.abs(out_d.numpy().astype(np.float64) - R.model64(iterates, 0.9)[-1]['m']) <= R.model64(iterates, 0.9)[-1]['e_m'])
    assert np.all(np.abs(torch.cat([t.reshape(-1) for t in out_c]).numpy() - out_d.numpy()) <= 2 * R.model64(iterates, 0.9)[-1]['e_m'])


def _state():
    return {'shadow': {'a0': torch.ones(5, 7), 'a1': torch.ones(11), 'a2': torch.ones(())}, 'decay': 0.9, 'updates': 3}


def _with(**kw):
    st = _state()
    st.update(kw)
    return st


def _shadow(**kw):
    st = _state()
    st['shadow'].update(kw)
    return st


STATE_REFUSALS = [
    ('no shadow', lambda: {k: v for k, v in _state().items() if k != 'shadow'}, "^ema: no 'shadow'"),
    ('no decay', lambda: {k: v for k, v in _state().items() if k != 'decay'}, "^ema: no 'decay'"),
    ('no updates', lambda: {k: v for k, v in _state().items() if k != 'updates'}, "^ema: no 'updates'"),
    ('no dict', lambda: [1, 2], '^ema: no'),
    ('decay 1', lambda: _with(decay=1.0), '^decay: '), ('decay negative', lambda: _with(decay=-0.5), '^decay: '),
    ('decay nan', lambda: _with(decay=NAN), '^decay: '), ('decay bool', lambda: _with(decay=True), '^decay: '),
    ('decay int', lambda: _with(decay=0), '^decay: '),
    ('updates negative', lambda: _with(updates=-1), '^updates: '), ('updates float', lambda: _with(updates=3.0), '^updates: '),
    ('updates bool', lambda: _with(updates=True), '^updates: '),
    ('updates 0 with a shadow', lambda: _with(updates=0), '^updates: 0 updates'),
    ('missing name', lambda: {**_state(), 'shadow': {k: v for k, v in _state()['shadow'].items() if k != 'a1'}}, r"^shadow: .*missing in the state \['a1'\]"),
    ('extra name', lambda: _shadow(b9=torch.ones(2)), r"^shadow: .*not in this model \['b9'\]"),
    ('order', lambda: {**_state(), 'shadow': dict(reversed(list(_state()['shadow'].items())))}, '^shadow: .*another order'),
    ('shape', lambda: _shadow(a1=torch.ones(12)), r"^shadow\['a1'\]: shape \(12,\)"),
    ('dtype', lambda: _shadow(a1=torch.ones(11, dtype=torch.float64)), r"^shadow\['a1'\]: .*float64"),
    ('no tensor', lambda: _shadow(a1=[1.0] * 11), r"^shadow\['a1'\]: shape list"),
    ('nan', lambda: _shadow(a0=torch.full((5, 7), NAN)), r"^shadow\['a0'\]: NaN or infinite"),
    ('inf', lambda: _shadow(a2=torch.tensor(float('inf'))), r"^shadow\['a2'\]: NaN or infinite"),
]


@pytest.mark.parametrize('what,make,match', STATE_REFUSALS, ids=[r[0] for r in STATE_REFUSALS])
def test_check_state_refuses_by_field_name(what, make, match):
    from qtmpnn.ema import WeightEMA, check_state
    table = [('a0', 0, (5, 7)), ('a1', 35, (11,)), ('a2', 46, ())]
    check_state(_state(), table)
    assert WeightEMA.check_state is check_state
    with pytest.raises(ValueError, match=match):
        check_state(make(), table)


# -- the predictor: refusals before anything runs ---------------------------------------------------------------------------------
@pytest.fixture
def cpu_predictor(monkeypatch, tmp_path):
    """A predictor without a device that records what would run (tests/test_validation_host.py's)."""
    from model.mpnnlstm import NextFramePredictorS2S
    from model.seq2seq import Seq2Seq
    from qtmpnn import _lib
    monkeypatch.chdir(tmp_path)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))
    nfp.ran = []
    record = lambda what: lambda *a, **k: nfp.ran.append(what)
    monkeypatch.setattr(nfp, 'train_step', record('train_step'))
    monkeypatch.setattr(nfp, '_inference', record('_inference'))
    monkeypatch.setattr(Seq2Seq, 'forward', record('forward'))
    monkeypatch.setattr(_lib, 'call', record('call'))
    monkeypatch.setattr(_lib, 'load', record('load'))
    return nfp


def _loader(n=2):
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(T_, 64, 64, 1)
    return TinyLoader([(x[None], y[None], torch.zeros(1))] * n, (64, 64))


BAD_DECAYS = [(True, TypeError), (False, TypeError), ('0.9', TypeError), ([0.9], TypeError), (1.0, ValueError), (1, ValueError),
              (-0.1, ValueError), (NAN, ValueError), (float('inf'), ValueError)]


@pytest.mark.parametrize('bad,error', BAD_DECAYS, ids=[repr(b) for b, _ in BAD_DECAYS])
def test_a_bad_decay_is_refused_by_name_before_anything_runs(cpu_predictor, bad, error):
    nfp = cpu_predictor
    with pytest.raises(error, match='^ema: '):
        nfp.train(_loader(), _loader(), n_epochs=1, ema=bad)
    assert nfp.ran == [] and not nfp.training_initiated and nfp.ema is None
    with pytest.raises(error, match='^ema: '):
        nfp.set_ema(bad)                    # (before the complaint about the missing optimiser)
    nfp.initiate_training(0.01, 0.5)
    with pytest.raises(error, match='^ema: '):
        nfp.set_ema(bad)
    assert nfp.ran == [] and nfp.ema is None


def test_ema_eval_and_the_other_refusals(cpu_predictor):
    nfp = cpu_predictor
    for bad in (1, None, 'yes', 0.0):
        with pytest.raises(TypeError, match='^ema_eval: '):
            nfp.train(_loader(), _loader(), n_epochs=1, ema=0.9, ema_eval=bad)
    for given in (True, False):
        with pytest.raises(ValueError, match='^ema_eval: '):
            nfp.train(_loader(), _loader(), n_epochs=1, ema_eval=given)
    with pytest.raises(ValueError, match='^ema: .*initiate_training'):
        nfp.set_ema(0.9)
    with pytest.raises(ValueError, match='^ema: averaged_weights'):
        with nfp.averaged_weights():
            pass
    with pytest.raises(ValueError, match='^ema: apply_ema'):
        nfp.apply_ema()
    assert nfp.ran == [] and not nfp.training_initiated and nfp.ema is None
    nfp.set_ema(None)                       # switching off what is off needs nothing
    nfp.initiate_training(0.01, 0.5)
    nfp.set_ema(0.9)
    before = [p.detach().clone() for p in nfp.model.parameters()]
    with pytest.raises(ValueError, match='^ema: no optimiser step has been averaged yet'):
        with nfp.averaged_weights():
            pass
    with pytest.raises(ValueError, match='^ema: no optimiser step has been averaged yet'):
        nfp.apply_ema()
    assert all(torch.equal(p, q) for p, q in zip(nfp.model.parameters(), before)) and nfp.ran == []


def test_set_ema_keeps_starts_and_drops_the_state(cpu_predictor):
    from qtmpnn.ema import WeightEMA
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    assert nfp.ema is None
    nfp.set_ema(0.9)
    first = nfp.ema
    assert isinstance(first, WeightEMA) and first.decay == 0.9 and first.updates == 0 and not first.flat
    first.update()
    nfp.set_ema(0.9)
    assert nfp.ema is first and first.updates == 1, 'the same decay keeps the state'
    nfp.set_ema(np.float64(0.9))
    assert nfp.ema is first
    nfp.set_ema(0.99)
    assert nfp.ema is not first and nfp.ema.updates == 0 and nfp.ema.decay == 0.99, 'another decay starts anew'
    nfp.set_ema(None)
    assert nfp.ema is None
    nfp.set_ema(0.5)
    nfp.initiate_training(0.01, 0.5)
    assert nfp.ema is None, 'initiate_training drops the average with the optimiser'
    assert nfp.ran == []


def _stepper(nfp, taken=0):
    """An optimiser step with fixed random gradients through _clip_and_step, the place every step goes through; taken: the steps
    another predictor's stepper has drawn gradients for already."""
    g = torch.Generator().manual_seed(4)
    for _ in range(taken):
        [torch.randn(p.shape, generator=g) for p in nfp.model.parameters()]

    def step():
        for p in nfp.model.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        nfp._clip_and_step(list(nfp.model.parameters()), 10.0)
    return step


def test_every_step_updates_once_and_the_block_swaps_the_weights(cpu_predictor):
    nfp = cpu_predictor
    nfp.initiate_training(0.01, 0.5)
    step = _stepper(nfp)
    step()
    assert nfp.ema is None
    nfp.set_ema(0.9)
    iterates = []
    for _ in range(4):
        step()
        iterates.append(np.concatenate([p.detach().numpy().reshape(-1) for p in nfp.model.parameters()]))
    assert nfp.ema.updates == 4
    ref = R.model64(iterates, 0.9)[-1]
    flat = lambda ts: np.concatenate([t.detach().numpy().reshape(-1) for t in ts])
    assert R.holds(flat(nfp.ema.shadow), None, ref)
    live = [p.detach().clone() for p in nfp.model.parameters()]
    with nfp.averaged_weights() as inside:
        assert inside is nfp
        assert R.holds(None, flat(nfp.model.parameters()), ref)
        assert not np.array_equal(flat(nfp.model.parameters()), flat(live))
        assert all(p.requires_grad for p in nfp.model.parameters())
        with pytest.raises(RuntimeError, match='^ema: averaged_weights.*re-entrant'):
            with nfp.averaged_weights():
                pass
        assert R.holds(None, flat(nfp.model.parameters()), ref), 'the refused nested block did not put the live weights back'
        for refused in (step, lambda: nfp.set_ema(None), nfp.apply_ema, lambda: nfp.save_checkpoint('x.pt')):
            with pytest.raises(RuntimeError, match='^ema: '):
                refused()
        assert nfp.ema.updates == 4
    assert all(torch.equal(p, q) for p, q in zip(nfp.model.parameters(), live)), 'bit for bit what they were'
    with pytest.raises(KeyError, match='inside'):
        with nfp.averaged_weights():
            raise KeyError('inside')
    assert all(torch.equal(p, q) for p, q in zip(nfp.model.parameters(), live)) and not nfp._ema_inside
    stash = [s.data_ptr() for s in nfp._ema_stash]
    with nfp.averaged_weights():
        pass
    assert stash == [s.data_ptr() for s in nfp._ema_stash], 'the stash is allocated once'
    nfp.apply_ema()
    assert R.holds(None, flat(nfp.model.parameters()), ref) and nfp.ema.updates == 4
    assert nfp.ran == []


def test_train_keeps_its_signature_and_takes_the_two_keywords(cpu_predictor):
    from model.mpnnlstm import NextFramePredictorS2S as P
    names = list(inspect.signature(P.train).parameters)
    assert names[-2:] == ['loss_weights', 'lead_weights'] and len(names) == 22 and 'ema' not in names
    assert list(inspect.signature(P.set_ema).parameters) == ['self', 'decay']
    assert list(inspect.signature(P.averaged_weights).parameters) == ['self'] and list(inspect.signature(P.apply_ema).parameters) == ['self']
    assert 'ema=decay' in P.train.__doc__ and 'ema_eval' in P.train.__doc__
    from qtmpnn import _lib
    assert len(_lib.exported_names()) == 91
    with pytest.raises(TypeError, match='emma'):
        cpu_predictor.train(_loader(), _loader(), n_epochs=1, emma=0.9)


# -- train()'s bookkeeping with an average, around a scripted test pass -----------------------------------------------------------
def _scripted(monkeypatch, tmp_path, losses):
    """tests/test_validation_host.py's: a CPU predictor whose training step adds 1 to every parameter -- through _clip_and_step,
    so that the average follows -- and whose test pass records the level of the weights it sees and returns the scripted sums."""
    from model.mpnnlstm import NextFramePredictorS2S
    monkeypatch.chdir(tmp_path)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.zero_()
    script, nfp.seen = iter(losses), []

    def train_step(*a, **k):
        with torch.no_grad():
            for p in nfp.model.parameters():
                p.add_(1.0)
        if nfp.ema is not None:
            nfp.ema.update()
        return torch.tensor(0.5)

    def test_pass(loader, climatology, loss_reduce, made, use_graph, graphed, **fwd):
        nfp.seen.append(_level(nfp))
        return 2 * next(script), 1
    monkeypatch.setattr(nfp, 'train_step', train_step)
    monkeypatch.setattr(nfp, '_test_pass', test_pass)
    return nfp


def _level(nfp):
    values = {round(float(v), 5) for p in nfp.model.parameters() for v in p.detach().reshape(-1)[:2]}
    assert len(values) == 1
    return values.pop()


def _mean(d, t):
    """The debiased average of the levels 1..t."""
    s = 0.0
    for i in range(1, t + 1):
        s = d * s + (1 - d) * i
    return round(s / (1 - d ** t), 5)


def test_the_test_pass_sees_the_averaged_weights_and_training_does_not(monkeypatch, tmp_path):
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.375])
    nfp.train(_loader(), _loader(1), n_epochs=3, truncated_backprop=0, ema=0.5)
    assert nfp.seen == [_mean(0.5, 2), _mean(0.5, 4), _mean(0.5, 6)] and nfp.seen[0] == round(5 / 3, 5)
    assert _level(nfp) == 6.0 and nfp.ema.updates == 6 and nfp.test_loss == [0.5, 0.25, 0.375]
    # ema_eval=False only maintains the average
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.125])
    nfp.train(_loader(), _loader(1), n_epochs=2, truncated_backprop=0, ema=0.5, ema_eval=False)
    assert nfp.seen == [2.0, 4.0] and nfp.ema.updates == 4
    # a later call without ema= keeps the setting and goes on averaging; ema_eval is then allowed
    nfp.train(_loader(), _loader(1), n_epochs=1, truncated_backprop=0, ema_eval=True)
    assert nfp.seen[-1] == _mean(0.5, 6) and nfp.ema.updates == 6 and _level(nfp) == 6.0


def test_restore_best_writes_the_weights_the_test_pass_saw(monkeypatch, tmp_path):
    nfp = _scripted(monkeypatch, tmp_path, [0.5, 0.25, 0.375, 0.3125])
    path = tmp_path / 'best.pt'
    nfp.train(_loader(), _loader(1), n_epochs=4, truncated_backprop=0, ema=0.5, restore_best=True, keep_best=path)
    assert (nfp.best_epoch, nfp.best_value) == (1, 0.25)
    assert _level(nfp) == _mean(0.5, 4), 'the averaged weights of epoch 1, neither its live ones (4.0) nor the last epoch\'s'
    ckpt = torch.load(path, weights_only=True)
    assert ckpt['format'] == 2 and ckpt['ema']['updates'] == 4 and ckpt['test_loss'] == [0.5, 0.25]
    first = next(iter(ckpt['state_dict'].values())).reshape(-1)[0].item()
    assert first == 4.0, 'keep_best writes an ordinary checkpoint: the live weights, with the average beside them'


# -- the checkpoint file ----------------------------------------------------------------------------------------------------------
def _trained(tmp_path, monkeypatch, decay):
    from model.mpnnlstm import NextFramePredictorS2S
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=3, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=1))
    nfp.initiate_training(0.01, 0.5)
    nfp.set_ema(decay)
    step = _stepper(nfp)
    for _ in range(3):
        step()
    nfp.train_loss, nfp.test_loss = [0.5], [0.75]
    return nfp, step


FORMAT_1 = {'format', 'description', 'state_dict', 'optimizer', 'scheduler', 'train_loss', 'test_loss', 'capturable', 'rng'}


def test_checkpoint_formats(tmp_path, monkeypatch):
    from model import mpnnlstm
    assert mpnnlstm.CHECKPOINT_FORMAT == 2
    off, _ = _trained(tmp_path, monkeypatch, None)
    off.save_checkpoint(tmp_path / 'off.pt')
    ckpt = torch.load(tmp_path / 'off.pt', weights_only=True)
    assert ckpt['format'] == 1 and set(ckpt) == FORMAT_1, 'without an average the file is what it was'
    on, step = _trained(tmp_path, monkeypatch, 0.9)
    on.save_checkpoint(tmp_path / 'on.pt')
    ckpt = torch.load(tmp_path / 'on.pt', weights_only=True)
    assert ckpt['format'] == 2 and set(ckpt) == FORMAT_1 | {'ema'}
    ema = ckpt['ema']
    assert set(ema) == {'shadow', 'decay', 'updates'} and ema['decay'] == 0.9 and ema['updates'] == 3
    assert list(ema['shadow']) == [n for n, _ in on.model.named_parameters()]
    assert all(torch.equal(t, s) for t, s in zip(ema['shadow'].values(), on.ema.shadow))
    for (n, p), q in zip(off.model.named_parameters(), on.model.parameters()):
        assert torch.equal(p, q), f'{n}: the average does not touch the run'

    # a fresh predictor gets the average from the file and continues it, bit for bit
    from model.mpnnlstm import NextFramePredictorS2S
    b = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=3, output_timesteps=3, device=None,
                              model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1, n_conv_layers=1))
    b.load_checkpoint(tmp_path / 'on.pt')
    assert b.ema is not None and b.ema.decay == 0.9 and b.ema.updates == 3
    assert all(torch.equal(s, t) for s, t in zip(b.ema.shadow, on.ema.shadow))
    step_b = _stepper(b, taken=3)
    step()
    step_b()
    assert b.ema.updates == on.ema.updates == 4
    assert all(torch.equal(s, t) for s, t in zip(b.ema.shadow, on.ema.shadow))
    assert all(torch.equal(p, q) for p, q in zip(b.model.parameters(), on.model.parameters()))
    # an average of the file's decay is loaded in place; another decay gives way to the file's; a file without one switches it off
    kept, ptrs = b.ema, [s.data_ptr() for s in b.ema.shadow]
    b.load_checkpoint(tmp_path / 'on.pt')
    assert b.ema is kept and ptrs == [s.data_ptr() for s in b.ema.shadow] and b.ema.updates == 3
    b.set_ema(0.5)
    b.load_checkpoint(tmp_path / 'on.pt')
    assert b.ema.decay == 0.9 and b.ema.updates == 3 and b.ema is not kept
    b.load_checkpoint(tmp_path / 'off.pt')
    assert b.ema is None


def _edit(path, out, fn):
    ckpt = torch.load(path, weights_only=True)
    fn(ckpt)
    torch.save(ckpt, out)
    return out


def _first(c):
    return next(iter(c['ema']['shadow']))


FILE_REFUSALS = [
    ('format 2 without ema', 'off.pt', '^format: .*format 2 and no \'ema\'', lambda c: c.__setitem__('format', 2)),
    ('format 1 with ema', 'on.pt', '^ema: averaged weights in a file of format 1', lambda c: c.__setitem__('format', 1)),
    ('format 3', 'on.pt', '^format: .*reads up to 2', lambda c: c.__setitem__('format', 3)),
    ('decay', 'on.pt', '^decay: ', lambda c: c['ema'].__setitem__('decay', 1.0)),
    ('updates', 'on.pt', '^updates: ', lambda c: c['ema'].__setitem__('updates', -2)),
    ('nan', 'on.pt', r'^shadow\[.*\]: NaN', lambda c: c['ema']['shadow'][_first(c)].view(-1)[0].fill_(NAN)),
    ('shape', 'on.pt', r'^shadow\[.*\]: shape', lambda c: c['ema']['shadow'].__setitem__(_first(c), torch.zeros(2, 2))),
    ('names', 'on.pt', '^shadow: parameter names differ', lambda c: c['ema']['shadow'].pop(_first(c))),
]


@pytest.mark.parametrize('what,source,match,edit', FILE_REFUSALS, ids=[r[0] for r in FILE_REFUSALS])
def test_a_file_that_does_not_fit_is_refused_by_name_and_changes_nothing(tmp_path, monkeypatch, what, source, match, edit):
    off, _ = _trained(tmp_path, monkeypatch, None)
    off.save_checkpoint(tmp_path / 'off.pt')
    on, step = _trained(tmp_path, monkeypatch, 0.9)
    on.save_checkpoint(tmp_path / 'on.pt')
    bad = _edit(tmp_path / source, tmp_path / 'bad.pt', edit)
    step()
    params, shadow, t = [p.detach().clone() for p in on.model.parameters()], [s.clone() for s in on.ema.shadow], on.ema.updates
    with pytest.raises(ValueError, match=match):
        on.load_checkpoint(bad)
    assert all(torch.equal(p, q) for p, q in zip(on.model.parameters(), params))
    assert all(torch.equal(s, q) for s, q in zip(on.ema.shadow, shadow)) and on.ema.updates == t == 4
