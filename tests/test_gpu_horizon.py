"""The rollout horizon on the GPU (set_horizon, horizon(k), train(horizon=)).  The oracle of every case is the TWIN: a predictor
built with output_timesteps=k that holds the same weights (load_state_dict) and starts from the same generator state; while a
horizon k is in force the predictor built with 4 steps must give the twin's bits -- loss, gradients, parameters after optimiser
steps, predicted arrays, product sums, attention-dropout counters.  Comparisons are torch.equal / np.array_equal unless stated.

64 x 64 frames, hidden 8, one layer, 3 input steps, 3 clips with distinct launch dates (one clip for the 17-step case), built with
4 output steps.  k = 1, 2 lie below the built value, 4 is it, 6 lies above it (y then holds 6 steps) and 17 is the smallest count
that crosses the 16-step chunk of the rollout loss, score and event-scan launches."""
import functools

import numpy as np
import pytest
import torch

from helpers import TinyLoader, climatology_from_base, dev, grad_close

pytestmark = pytest.mark.gpu

T_IN, BUILT, LONG = 3, 4, 17
MASK = np.zeros((64, 64), dtype=bool)
MASK[:, 58:] = True
DAY = 86400 * 10 ** 9
DATES = torch.tensor([1356350400 * 10 ** 9 + DAY * i for i in (0, 3, 9, 20, 41, 77)], dtype=torch.int64)   # (from 2012-12-24)


@pytest.fixture(autouse=True)
def _quiet(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)             # (initiate_training()'s SummaryWriter writes under the working directory)


@functools.lru_cache(maxsize=None)
def _clips():
    """Six clips (x (6, 3, 64, 64, 1), y (6, 17, 64, 64, 1)) on the device, made once, not modified."""
    from qtmpnn import synthetic
    x, y = synthetic.make_batch(11, 0, 6, T_IN, LONG, n_digits=2, pixel_noise=0.02)
    return torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())


def _batch(steps, clips=slice(0, 3)):
    """(x, y with `steps` output steps) of some clips: y is a copy, so y with 4 steps is all a predictor built with 4 ever sees."""
    x, y = _clips()
    return x[clips].clone(), y[clips, :steps].clone()


@functools.lru_cache(maxsize=None)
def _climatology():
    base = np.random.default_rng(11).random((64, 64), dtype=np.float32)
    clim = climatology_from_base(base)
    return torch.from_numpy(np.concatenate([clim, clim[:, :1]], axis=1)).to(dev())         # (1, 366, 64, 64)


def _seed(seed=5):
    from qtmpnn import ops
    torch.manual_seed(seed)
    ops.set_dropout_state({'calls': 0, 'epoch': 0}, dev())


def _fresh(steps, conv='ChebConv', dropout=0.0, binary=False, seed=5):
    from model.mpnnlstm import NextFramePredictorS2S
    _seed(seed)
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=T_IN, output_timesteps=steps, device=dev(), binary=binary,
                                model_kwargs=dict(hidden_size=8, dropout=dropout, n_layers=1, n_conv_layers=1, convolution_type=conv))
    with torch.no_grad():
        for p in nfp.model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    nfp.model.eval()
    return nfp


def _pair(k, capturable=None, **kw):
    """(the predictor built with 4 steps, its twin built with k) with the same weights; capturable None: no optimiser yet."""
    main, twin = _fresh(BUILT, **kw), _fresh(k, **kw)
    twin.model.load_state_dict(main.model.state_dict())
    assert main.built_output_timesteps == BUILT and twin.output_timesteps == k
    if capturable is not None:
        for nfp in (main, twin):
            nfp.initiate_training(lr=0.01, lr_decay=0.5, capturable=capturable)
    return main, twin


def _same_params(a, b):
    for (name, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), name


def _loss_and_gradient(nfp, x, y, concat=None, **kw):
    nfp.zero_grad()
    loss = nfp.forward_loss(x, y, concat, MASK, **kw)
    loss.backward()
    return loss.detach().clone(), nfp._grad_flat().clone()


def _held(k):
    """The steps of y the predictor built with 4 is given under horizon k: what it was built for, more only where k needs more."""
    return max(k, BUILT)


# -- ChebConv: forward, loss, backward, optimiser steps; eager and captured -------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 4, 6])
def test_eager_loss_gradients_and_steps_are_the_twins(k):
    main, twin = _pair(k, capturable=False)
    (x, y), (_, yk) = _batch(_held(k)), _batch(k)
    with main.horizon(k):
        assert main.output_timesteps == k
        _seed()
        got = _loss_and_gradient(main, x, y)
        _seed()
        want = _loss_and_gradient(twin, x, yk)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool(torch.isfinite(got[0]))
        assert bool(got[1].any()), 'the gradient is not zero'
        for i in range(2):
            lm, lt = main.train_step(x, y, None, MASK), twin.train_step(x, yk, None, MASK)
            assert torch.equal(lm, lt), (i, lm, lt)
        _same_params(main, twin)
        # accumulated and truncated steps read the same setting
        lm, lt = main.accumulated_step([(x, y), (x[:2], y[:2])], MASK), twin.accumulated_step([(x, yk), (x[:2], yk[:2])], MASK)
        assert torch.equal(lm, lt)
        cm, ct = main.truncated_backward(x, y, None, MASK, truncated_backprop=2), twin.truncated_backward(x, yk, None, MASK, truncated_backprop=2)
        assert len(cm) == len(ct) == -(k // -2) and all(torch.equal(a, b) for a, b in zip(cm, ct))
        assert torch.equal(main._grad_flat(), twin._grad_flat())
        _same_params(main, twin)
    assert main.output_timesteps == BUILT
    if k != BUILT:      # the setting matters: without it the same predictor rolls out four steps, another loss
        assert not torch.equal(_loss_and_gradient(main, x, y[:, :BUILT].contiguous())[0], got[0])


@pytest.mark.parametrize('k', [1, 2, 4, 6])
def test_captured_steps_are_the_twins(k):
    main, twin = _pair(k, capturable=True)
    (x, y), (_, yk) = _batch(_held(k)), _batch(k)
    with main.horizon(k):
        step = main.make_graphed_step(x, y, None, MASK, warmup=1)
    want = twin.make_graphed_step(x, yk, None, MASK, warmup=1)
    assert step.horizon == k and torch.equal(main.last_warmup_loss, twin.last_warmup_loss)
    (x2, y2), (_, y2k) = _batch(_held(k), slice(3, 6)), _batch(k, slice(3, 6))
    for i, (a, b, bk) in enumerate(((x2, y2, y2k), (x, y, yk))):
        lm, lt = step(a, b), want(a, bk)
        assert torch.equal(lm, lt) and bool(torch.isfinite(lm)), (i, lm, lt)
    _same_params(main, twin)
    # accumulate=2 under the same horizon
    with main.horizon(k):
        acc = main.make_graphed_step(x, y, None, MASK, warmup=1, accumulate=2)
    want = twin.make_graphed_step(x, yk, None, MASK, warmup=1, accumulate=2)
    assert acc.horizon == k
    lm, lt = acc([(x2, y2), (x, y)]), want([(x2, y2k), (x, yk)])
    assert torch.equal(lm, lt)
    _same_params(main, twin)
    main.model.static_shapes = twin.model.static_shapes = False


def test_a_captured_step_keeps_the_horizon_it_was_captured_under():
    main, twin = _pair(2, capturable=True)
    (x, y), (_, yk) = _batch(BUILT), _batch(2)
    with main.horizon(2):
        step = main.make_graphed_step(x, y, None, MASK, warmup=1)
    want = twin.make_graphed_step(x, yk, None, MASK, warmup=1)
    main.set_horizon(None)
    assert main.output_timesteps == BUILT and step.horizon == 2
    for other in (None, 3, 6):          # whatever is set by now, the replay runs two steps
        main.set_horizon(other)
        assert torch.equal(step(x, y), want(x, yk))
    main.set_horizon(None)
    _same_params(main, twin)
    before = [p.detach().clone() for p in main.model.parameters()]
    with pytest.raises(ValueError, match='^horizon: y holds 1 output steps, horizon=2 needs 2$'):
        step(x, y[:, :1])
    assert all(torch.equal(p, q) for p, q in zip(main.model.parameters(), before)), 'the refused replay ran nothing'
    assert torch.equal(step(x, y[:, :2]), want(x, yk)), 'y with exactly the captured steps'
    main.model.static_shapes = twin.model.static_shapes = False


# -- across the 16-step chunk -----------------------------------------------------------------------------------------------------
def test_seventeen_steps_cross_the_chunk_of_the_loss_score_and_event_launches():
    from model.mpnnlstm import DEFAULT_PRODUCTS
    main, twin = _pair(LONG, capturable=False)
    x, y = _batch(LONG, slice(0, 1))
    with main.horizon(LONG):
        _seed()
        got = _loss_and_gradient(main, x, y)
        _seed()
        want = _loss_and_gradient(twin, x, y)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool(torch.isfinite(got[0]))
        loader = TinyLoader([(x.cpu(), y.cpu(), DATES[:1])], (64, 64))
        vm, vt = main.verify(loader, mask=MASK), twin.verify(loader, mask=MASK)
    assert vm.products == vt.products == DEFAULT_PRODUCTS
    for name in DEFAULT_PRODUCTS:
        assert vm[name].sums.shape == vt[name].sums.shape and np.array_equal(vm[name].sums, vt[name].sums, equal_nan=True), name
        if name != 'event_dates':
            assert vm[name].sums.shape[:2] == (1, LONG), name
    assert np.array_equal(vm.event_dates.dates, vt.event_dates.dates)


# -- attention with dropout: the counters afterwards --------------------------------------------------------------------------------
def test_transformer_with_dropout_leaves_the_twins_counters():
    from qtmpnn import ops
    main, twin = _pair(2, capturable=False, conv='TransformerConv', dropout=0.1)
    main.model.train(), twin.model.train()
    (x, y), (_, yk) = _batch(BUILT), _batch(2)
    results = []
    for nfp, targets, setting in ((main, y, 2), (twin, yk, None)):
        _seed()
        nfp.set_horizon(setting)
        passes = [_loss_and_gradient(nfp, x, targets) for _ in range(2)]            # (a counter left wrong shows in the second)
        results.append((passes, dict(ops.dropout_state(dev()))))
    (pm, cm), (pt, ct) = results
    assert cm == ct and cm['calls'] > 0, (cm, ct)
    for i, ((lm, gm), (lt, gt)) in enumerate(zip(pm, pt)):
        assert torch.equal(lm, lt) and torch.equal(gm, gt), i
    assert not torch.equal(pm[0][0], pm[1][0]), 'the two passes draw different masks'
    # four steps advance the counters further: the counters do tell the horizons apart
    _seed()
    main.set_horizon(None)
    _loss_and_gradient(main, x, y), _loss_and_gradient(main, x, y)
    assert dict(ops.dropout_state(dev())) != cm


# -- binary head, captured ------------------------------------------------------------------------------------------------------------
def test_binary_captured_step_is_the_twins():
    main, twin = _pair(2, capturable=True, binary=True)
    x, y = _batch(BUILT)
    y = (y > 0.3).float()
    yk = y[:, :2].contiguous()
    with main.horizon(2):
        step = main.make_graphed_step(x, y, None, MASK, warmup=1)
    want = twin.make_graphed_step(x, yk, None, MASK, warmup=1)
    assert torch.equal(main.last_warmup_loss, twin.last_warmup_loss)
    for _ in range(2):
        lm, lt = step(x, y), want(x, yk)
        assert torch.equal(lm, lt) and bool(torch.isfinite(lm))
    _same_params(main, twin)
    main.model.static_shapes = twin.model.static_shapes = False


# -- masked frames with a batched climatology: predict and verify as captured graphs ---------------------------------------------------
@pytest.mark.parametrize('k', [2, 6])
def test_graphed_predict_and_verify_with_a_batched_climatology(k):
    main, twin = _pair(k)
    clim = _climatology()
    (x, y), (_, yk) = _batch(_held(k)), _batch(k)
    loader = TinyLoader([(x.cpu(), y.cpu(), DATES[:3]), (x.flip(0).cpu(), y.flip(0).cpu(), DATES[3:])], (64, 64))
    twins = TinyLoader([(x.cpu(), yk.cpu(), DATES[:3]), (x.flip(0).cpu(), yk.flip(0).cpu(), DATES[3:])], (64, 64))
    products = {'score': None, 'event_dates': dict(persist=2)}
    with main.horizon(k):
        assert tuple(main.get_climatology_array(clim, DATES[:3]).shape) == (3, k, 64, 64, 1)
        pm = main.predict(loader, clim, mask=MASK, use_graph=True)
        vm = main.verify(loader, clim, mask=MASK, use_graph=True, products=products)
        with pytest.raises(ValueError, match=f'persist must be an integer in 1..{k} '):
            main.verify(loader, clim, mask=MASK, products={'event_dates': dict(persist=k + 1)})
    pt = twin.predict(twins, clim, mask=MASK, use_graph=True)
    vt = twin.verify(twins, clim, mask=MASK, use_graph=True, products=products)
    assert pm.shape == pt.shape == (6, k, 64, 64, 1) and pm[0].shape == (k, 64, 64, 1) and np.array_equal(pm, pt, equal_nan=True)
    assert vm.score.sums.shape == (6, k, 3, 8), 'k leads'
    assert np.array_equal(vm.score.sums, vt.score.sums) and vm.sources == vt.sources == ('model', 'persistence', 'climatology')
    assert np.array_equal(vm.event_dates.dates, vt.event_dates.dates) and np.array_equal(vm.event_dates.sums, vt.event_dates.sums)
    assert not main.model.static_shapes and main.output_timesteps == BUILT
    # eagerly as well, with the same numbers for the score
    with main.horizon(k):
        ve = main.verify(loader, clim, mask=MASK, products=products)
    assert np.array_equal(ve.score.sums, vt.score.sums) and np.array_equal(ve.event_dates.dates, vt.event_dates.dates)


def test_a_captured_product_keeps_its_horizon():
    main, twin = _pair(2)
    (x, y), (_, yk) = _batch(BUILT), _batch(2)
    with main.horizon(2):
        scores = main.make_graphed_scores(x, y, None, MASK)
    want = twin.make_graphed_scores(x, yk, None, MASK)
    assert tuple(scores.warmup.shape) == (2, 3, 2, 8) and torch.equal(scores.warmup, want.warmup)
    assert torch.equal(scores(x.flip(0), y.flip(0)), want(x.flip(0), yk.flip(0)))           # (set_horizon(None) by now)
    with pytest.raises(ValueError, match='^horizon: y holds 1 output steps, horizon=2 needs 2$'):
        scores(x, y[:, :1])
    main.model.static_shapes = twin.model.static_shapes = False


# -- recompute mode 'stream' ------------------------------------------------------------------------------------------------------------
def test_stream_recompute_under_a_horizon():
    main, twin = _pair(2, capturable=False)
    (x, y), (_, yk) = _batch(BUILT), _batch(2)
    plain = _loss_and_gradient(twin, x, yk)
    main.set_recompute('stream'), twin.set_recompute('stream')
    with main.horizon(2):
        got = _loss_and_gradient(main, x, y)
        outs_m = [o.detach().clone() for o in main.model(x, y[:, :2], None, teacher_forcing_ratio=0, mask=MASK)[0]]
    want = _loss_and_gradient(twin, x, yk)
    outs_t = [o.detach().clone() for o in twin.model(x, yk, None, teacher_forcing_ratio=0, mask=MASK)[0]]
    assert torch.equal(got[0], want[0]) and torch.equal(got[0], plain[0])
    assert len(outs_m) == len(outs_t) == 2 and all(torch.equal(a, b) for a, b in zip(outs_m, outs_t))
    # 'stream' sums the weight gradients in another order: up to rounding, tests/test_gpu_stream.py's bound
    grad_close(got[1], want[1], msg='stream, horizon against twin')
    grad_close(got[1], plain[1], msg='stream against the plain twin')
    # 'step' promises the bits
    main.set_recompute('step'), twin.set_recompute('step')
    with main.horizon(2):
        got = _loss_and_gradient(main, x, y)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])


def test_sensitivity_and_attention_weights_follow_the_horizon():
    main, twin = _pair(2)
    x, _ = _batch(BUILT)
    with main.horizon(2):
        sm = main.sensitivity(x[:2], mask=MASK)
        with pytest.raises(ValueError, match='leads'):
            main.sensitivity(x[:2], mask=MASK, leads=[2])
    st = twin.sensitivity(x[:2], mask=MASK)
    assert sm.maps.shape == st.maps.shape and sm.maps.shape[1] == 2 and np.array_equal(sm.maps, st.maps) and np.array_equal(sm.J, st.J)
    am, at = _pair(2, conv='TransformerConv')
    with am.horizon(2):
        rm = am.attention_weights(x[:1], mask=MASK)
    rt = at.attention_weights(x[:1], mask=MASK)
    assert len(rm) == len(rt) and max(r['t'] for r in rm if r['phase'] == 'decoder') == 1
    assert all(torch.equal(a['alpha'], b['alpha']) for a, b in zip(rm, rt))


# -- the curriculum -----------------------------------------------------------------------------------------------------------------
def _loaders():
    """(train: 2 batches of 2 clips, test: 1 batch of 2 clips), y of 4 steps, on the host."""
    x, y = (t.cpu() for t in _clips())
    item = lambda a: (x[a:a + 2].clone(), y[a:a + 2, :BUILT].clone(), DATES[a:a + 2])
    return TinyLoader([item(0), item(2)], (64, 64)), TinyLoader([item(4)], (64, 64))


def _moments(nfp):
    from qtmpnn.optim import adam_state
    state = adam_state(nfp.optimizer, nfp.model)
    return [state['step']] + [t for key in ('exp_avg', 'exp_avg_sq') for t in state[key].values()]


def _same_training_state(a, b):
    assert a.train_loss == b.train_loss and a.test_loss == b.test_loss, (a.train_loss, b.train_loss, a.test_loss, b.test_loss)
    _same_params(a, b)
    for i, (s, t) in enumerate(zip(_moments(a), _moments(b))):
        assert torch.equal(torch.as_tensor(s), torch.as_tensor(t)), i
    assert float(a.optimizer.param_groups[0]['lr']) == float(b.optimizer.param_groups[0]['lr'])


def _hand_loop(nfp, schedule, use_graph):
    """What train(horizon=schedule, truncated_backprop=0) is to do, written out: per epoch the training batches under
    horizon(k_e) -- train_step, or the step captured under k_e, whose one warm-up step is the first batch's own update -- then the
    test pass at the built horizon, then scheduler.step()."""
    train, test = _loaders()
    nfp.initiate_training(0.01, 0.5, capturable=use_graph)
    on = lambda t: t.to(dev())
    steps = {}
    for k in schedule:
        losses, steps = [], {kept: step for kept, step in steps.items() if kept == k}      # (a horizon the schedule left is dropped)
        step = steps.get(k)
        with nfp.horizon(k):
            for x, y, _ in train:
                if not use_graph:
                    losses.append(nfp.train_step(on(x), on(y), None, MASK).item())
                elif step is None:
                    step = steps[k] = nfp.make_graphed_step(on(x), on(y), None, mask=MASK, warmup=1, max_norm=10.0)
                    losses.append(nfp.last_warmup_loss.item())
                else:
                    losses.append(step(on(x), on(y)).item())
        assert nfp.output_timesteps == BUILT
        tests = []
        with torch.no_grad():
            for x, y, _ in test:
                tests.append(nfp.forward_loss(on(x), on(y), None, MASK).item())
        nfp.scheduler.step()
        nfp.train_loss.append(sum(losses) / (len(losses) + 1))
        nfp.test_loss.append(sum(tests) / (len(tests) + 1))


@pytest.mark.parametrize('use_graph', [False, True])
def test_the_curriculum_is_the_hand_loop(use_graph):
    trained, by_hand = _fresh(BUILT), _fresh(BUILT)
    trained.train(*_loaders(), n_epochs=3, lr=0.01, lr_decay=0.5, mask=MASK, truncated_backprop=0, use_graph=use_graph, horizon=[1, 2])
    _hand_loop(by_hand, [1, 2, 2], use_graph)
    assert len(trained.train_loss) == 3 and trained.output_timesteps == BUILT
    _same_training_state(trained, by_hand)
    # the epochs differ: one step, then two; the test pass is the four-step loss throughout
    assert trained.train_loss[0] != trained.train_loss[1] and all(np.isfinite(trained.test_loss))
    trained.model.static_shapes = by_hand.model.static_shapes = False


def test_a_resumed_curriculum_ends_in_the_bits_of_the_uninterrupted_run():
    kw = dict(lr=0.01, lr_decay=0.5, mask=MASK, truncated_backprop=0, horizon=[1, 2])
    whole, first, second = _fresh(BUILT), _fresh(BUILT), _fresh(BUILT, seed=9)
    whole.train(*_loaders(), n_epochs=3, **kw)
    first.train(*_loaders(), n_epochs=1, **kw)
    first.save_checkpoint('epoch1.pt')
    second.load_checkpoint('epoch1.pt')
    assert second.output_timesteps == BUILT
    second.train(*_loaders(), n_epochs=2, **kw)               # (epochs 1 and 2 of the history: horizons 2 and 2)
    _same_training_state(whole, second)


def test_train_without_the_keyword_is_what_it_was():
    a, b, c = _fresh(BUILT), _fresh(BUILT), _fresh(BUILT)
    kw = dict(n_epochs=2, lr=0.01, lr_decay=0.5, mask=MASK)
    a.train(*_loaders(), **kw)
    b.train(*_loaders(), horizon=None, **kw)
    c.train(*_loaders(), horizon=BUILT, **kw)
    _same_training_state(a, b)
    _same_training_state(a, c)


# -- refusals that need a device batch: before any launch -----------------------------------------------------------------------------
def test_refusals_come_before_any_launch(monkeypatch):
    from qtmpnn import _lib
    main = _fresh(BUILT)
    main.initiate_training(0.01, 0.5)
    clim = _climatology()
    x, y = _batch(BUILT)
    concat = main.get_climatology_array(clim, DATES[:3])
    loader = TinyLoader([(x.cpu(), y.cpu(), DATES[:3])], (64, 64))
    launched, call = [], _lib.call
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a[0]) or call(*a))
    short_y = '^horizon: y holds 4 output steps, horizon=6 needs 6$'
    short_c = '^horizon: concat_layers holds 4 output steps, horizon=6 needs 6$'
    with main.horizon(6):
        y6 = _batch(6)[1]
        for refused, match in ((lambda: main.forward_loss(x, y, None, MASK), short_y), (lambda: main.train_step(x, y, None, MASK), short_y),
                               (lambda: main.make_graphed_step(x, y, None, MASK), short_y),
                               (lambda: main.make_graphed_scores(x, y, None, MASK), short_y),
                               (lambda: main.verify(loader, mask=MASK, products=('score',)), short_y),
                               (lambda: main.train(loader, loader, n_epochs=1, mask=MASK), short_y),
                               (lambda: main.forward_loss(x, y6, concat, MASK), short_c),
                               (lambda: main.make_graphed_rollout(x, concat, MASK), short_c),
                               (lambda: main.sensitivity(x, concat, MASK), short_c)):
            with pytest.raises(ValueError, match=match):
                refused()
            assert launched == [], launched
    # a schedule entry above the steps of the loader's y: on the first batch of that epoch, before its launch
    with pytest.raises(ValueError, match=short_y):
        main.train(loader, loader, n_epochs=1, mask=MASK, truncated_backprop=0, horizon=6)
    assert launched == [] and main.output_timesteps == BUILT and not main.model.static_shapes
    main.forward_loss(x, y, None, MASK)
    assert launched, 'the recorder sees the launches of a call that runs'
