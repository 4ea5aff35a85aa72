"""CPU-side checks of save_checkpoint() / load_checkpoint() (no GPU: the optimiser is torch's Adam and nothing reaches the qtmpnn
kernels): the round trip of every piece of state, the file's layout, every refusal by field name with the target left untouched,
the flat <-> per-name slicing, and the atomic write."""
import os

import pytest
import torch

STEPS = 3


def _predictor(seed=0, conv='ChebConv', hidden=8, binary=False, **kw):
    from model.mpnnlstm import NextFramePredictorS2S
    torch.manual_seed(seed)
    kw = dict(dict(input_features=1, input_timesteps=3, output_timesteps=3), **kw)
    return NextFramePredictorS2S(thresh=0.1, device=None, binary=binary,
                                 model_kwargs=dict(hidden_size=hidden, dropout=0.0, n_layers=1, n_conv_layers=1, convolution_type=conv), **kw)


def _grads(nfp, round_):
    """Fixed random gradients for round `round_`, the same for every predictor of the same shapes (a generator of their own)."""
    g = torch.Generator().manual_seed(1000 + round_)
    return [torch.randn(p.shape, generator=g) for p in nfp.model.parameters()]


def _step(nfp, round_):
    for p, g in zip(nfp.model.parameters(), _grads(nfp, round_)):
        p.grad = g.clone()
    nfp.optimizer.step()
    nfp.scheduler.step()


def _trained(tmp_path, monkeypatch, **kw):
    monkeypatch.chdir(tmp_path)             # (a SummaryWriter, where tensorboard is installed, writes runs/ under the cwd)
    nfp = _predictor(**kw)
    nfp.initiate_training(lr=0.01, lr_decay=0.5)
    for r in range(STEPS):
        _step(nfp, r)
    nfp.train_loss, nfp.test_loss = [0.5, 0.25, 0.125], [0.75, 0.5, 0.375]
    return nfp


def _snapshot(nfp):
    """Copies of everything a load may touch."""
    snap = {'p.' + k: v.detach().clone() for k, v in nfp.model.state_dict().items()}
    if nfp.training_initiated:
        for (name, p) in nfp.model.named_parameters():
            for k, v in nfp.optimizer.state.get(p, {}).items():
                snap[f'o.{name}.{k}'] = v.detach().clone()
        snap['lr'] = torch.tensor(float(nfp.optimizer.param_groups[0]['lr']), dtype=torch.float64)
        snap['last_epoch'] = torch.tensor(nfp.scheduler.last_epoch)
        snap['hist'] = torch.tensor(nfp.train_loss + nfp.test_loss, dtype=torch.float64)
    snap['initiated'] = torch.tensor(nfp.training_initiated)
    return snap


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_round_trip_and_continuation(tmp_path, monkeypatch):
    a = _trained(tmp_path, monkeypatch)
    path = tmp_path / 'a.ckpt'
    a.save_checkpoint(path)
    b = _predictor(seed=77)                 # other weights, not trained yet: the load initiates training itself
    torch.manual_seed(123)
    rng_a = torch.get_rng_state()
    torch.manual_seed(9)
    assert not b.training_initiated
    b.load_checkpoint(path)
    assert b.training_initiated and b.optimizer.param_groups[0]['capturable'] is False
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n
        sa, sb = a.optimizer.state[p], b.optimizer.state[q]
        for k in ('exp_avg', 'exp_avg_sq', 'step'):
            assert torch.equal(sa[k], sb[k]) and sa[k].dtype == sb[k].dtype, (n, k)
        assert float(sb['step']) == STEPS
    ga, gb = a.optimizer.param_groups[0], b.optimizer.param_groups[0]
    assert ga['lr'] == gb['lr'] == 0.005 and ga['initial_lr'] == gb['initial_lr'] == 0.01        # (StepLR moved at epoch 3)
    assert ga['betas'] == gb['betas'] and ga['eps'] == gb['eps']
    assert a.scheduler.last_epoch == b.scheduler.last_epoch == STEPS
    assert a.scheduler.state_dict() == b.scheduler.state_dict()
    assert b.scheduler.get_last_lr() == [0.005]
    assert (b.train_loss, b.test_loss) == (a.train_loss, a.test_loss) == ([0.5, 0.25, 0.125], [0.75, 0.5, 0.375])
    # the file was written with the generator at seed 0's state after building a; the load puts that state back
    assert not torch.equal(torch.get_rng_state(), rng_a)
    assert torch.equal(torch.get_rng_state(), torch.load(path, weights_only=True)['rng']['torch'])
    for r in range(STEPS, STEPS + 3):       # (3 more: the schedule moves again at epoch 6)
        _step(a, r)
        _step(b, r)
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n
    assert a.optimizer.param_groups[0]['lr'] == b.optimizer.param_groups[0]['lr'] == 0.0025


def test_weights_alone_do_not_continue_the_run(tmp_path, monkeypatch):
    """The comparison above can fail: save() / load() carry the weights only, and the continued parameters differ."""
    a = _trained(tmp_path, monkeypatch)
    a.save(str(tmp_path))
    b = _predictor(seed=77)
    b.load(str(tmp_path))
    b.initiate_training(lr=0.01, lr_decay=0.5)
    for r in range(STEPS, STEPS + 2):
        _step(a, r)
        _step(b, r)
    assert not all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))


def test_file_loads_safely_and_holds_the_weights_of_save(tmp_path, monkeypatch):
    a = _trained(tmp_path, monkeypatch)
    path = tmp_path / 'a.ckpt'
    a.save_checkpoint(path)
    a.save(str(tmp_path))
    ckpt = torch.load(path, weights_only=True)
    pth = torch.load(tmp_path / f'{a.experiment_name}.pth', weights_only=True)
    assert list(ckpt['state_dict']) == list(pth) and all(torch.equal(ckpt['state_dict'][k], pth[k]) for k in pth)
    assert ckpt['format'] == 1 and ckpt['capturable'] is False
    d = ckpt['description']
    assert {k: d[k] for k in d if k != 'parameters'} == dict(
        convolution_type='ChebConv', hidden_size=8, n_layers=1, n_conv_layers=1, input_features=1, input_timesteps=3, output_timesteps=3,
        binary=False)
    assert d['parameters'] == [[n, list(p.shape)] for n, p in a.model.named_parameters()]
    opt = ckpt['optimizer']
    assert set(opt) == {'exp_avg', 'exp_avg_sq', 'step', 'lr', 'betas', 'eps'}
    assert opt['step'] == STEPS and type(opt['step']) is int and opt['lr'] == 0.005 and type(opt['lr']) is float
    assert tuple(opt['betas']) == (0.9, 0.999) and opt['eps'] == 1e-8
    for n, p in a.model.named_parameters():
        assert torch.equal(opt['exp_avg'][n], a.optimizer.state[p]['exp_avg']) and opt['exp_avg'][n].shape == p.shape
        assert torch.equal(opt['exp_avg_sq'][n], a.optimizer.state[p]['exp_avg_sq'])
    s = ckpt['scheduler']
    assert (s['last_epoch'], s['_last_lr'], s['step_size'], s['gamma']) == (STEPS, [0.005], 3, 0.5)
    assert (ckpt['train_loss'], ckpt['test_loss']) == (a.train_loss, a.test_loss)
    assert ckpt['rng']['cuda'] is None and ckpt['rng']['torch'].dtype == torch.uint8
    assert set(ckpt['rng']['attention']) == {'calls', 'epoch'}

    def plain(v):
        if isinstance(v, dict):
            return all(isinstance(k, str) and plain(e) for k, e in v.items())
        if isinstance(v, (list, tuple)):
            return all(plain(e) for e in v)
        return v is None or isinstance(v, (bool, int, float, str)) or (torch.is_tensor(v) and v.device.type == 'cpu')
    assert plain(ckpt)


def test_capturable_conversion_on_the_host(tmp_path, monkeypatch):
    """load_checkpoint(capturable=True) of an eager file: lr becomes a tensor the scheduler updates in place, and back."""
    a = _trained(tmp_path, monkeypatch)
    path, path2 = tmp_path / 'a.ckpt', tmp_path / 'b.ckpt'
    a.save_checkpoint(path)
    b = _predictor(seed=5)
    b.load_checkpoint(path, capturable=True)
    g = b.optimizer.param_groups[0]
    assert g['capturable'] is True and torch.is_tensor(g['lr']) and float(g['lr']) == pytest.approx(0.005, rel=1e-7)
    assert b.scheduler._last_lr[0] is g['lr'] and torch.is_tensor(g['initial_lr'])
    lr0 = g['lr']
    b.save_checkpoint(path2)
    assert torch.load(path2, weights_only=True)['capturable'] is True
    b.load_checkpoint(path)                 # the stored flag is False: back to a float
    assert b.optimizer.param_groups[0]['capturable'] is False and b.optimizer.param_groups[0]['lr'] == 0.005
    b.load_checkpoint(path2)
    b.load_checkpoint(path2)                # same mode: in place, the lr tensor is the one the optimiser had
    g = b.optimizer.param_groups[0]
    assert torch.is_tensor(g['lr']) and g['lr'] is not lr0
    lr1, states = g['lr'], [b.optimizer.state[p] for p in b.model.parameters()]
    ptrs = [(s['exp_avg'].data_ptr(), s['step'].data_ptr()) for s in states]
    b.load_checkpoint(path2)
    assert b.optimizer.param_groups[0]['lr'] is lr1
    assert ptrs == [(b.optimizer.state[p]['exp_avg'].data_ptr(), b.optimizer.state[p]['step'].data_ptr()) for p in b.model.parameters()]


def _edit(path, out, fn):
    ckpt = torch.load(path, weights_only=True)
    fn(ckpt)
    torch.save(ckpt, out)
    return out


def _first(ckpt, key):
    return next(iter(ckpt['optimizer'][key]))


def _set(d, k, v):
    d[k] = v


def _rename(ckpt):
    for d in (ckpt['optimizer']['exp_avg'], ckpt['optimizer']['exp_avg_sq']):
        d['decoder.not_there'] = d.pop(next(iter(d)))
    ckpt['description']['parameters'][0][0] = 'decoder.not_there'


EDITS = [
    ('newer format', '^format:', lambda c: _set(c, 'format', 2)),
    ('another convolution', "convolution_type='GCNConv' in the file, 'ChebConv' here",
     lambda c: _set(c['description'], 'convolution_type', 'GCNConv')),
    ('another hidden size', 'hidden_size=16', lambda c: _set(c['description'], 'hidden_size', 16)),
    ('other output steps', 'output_timesteps=5', lambda c: _set(c['description'], 'output_timesteps', 5)),
    ('binary', 'binary=True', lambda c: _set(c['description'], 'binary', True)),
    ('extra and missing names', 'decoder.not_there', _rename),
    ('missing moment', 'exp_avg_sq: parameter names differ', lambda c: c['optimizer']['exp_avg_sq'].pop(_first(c, 'exp_avg_sq'))),
    ('parameter shape', r'parameters\[.*\]: shape', lambda c: _set(c['description']['parameters'][0], 1, [3, 3])),
    ('moment shape', r'exp_avg\[.*\]: shape',
     lambda c: _set(c['optimizer']['exp_avg'], _first(c, 'exp_avg'), torch.zeros(2, 2))),
    ('weight shape', r'state_dict\[.*\]: shape',
     lambda c: _set(c['state_dict'], next(iter(c['state_dict'])), torch.zeros(2, 2))),
    ('nan moment', r'exp_avg\[.*\]: NaN', lambda c: c['optimizer']['exp_avg'][_first(c, 'exp_avg')].view(-1)[0].fill_(float('nan'))),
    ('inf second moment', r'exp_avg_sq\[.*\]: NaN or infinite',
     lambda c: c['optimizer']['exp_avg_sq'][_first(c, 'exp_avg_sq')].view(-1)[0].fill_(float('inf'))),
    ('negative second moment', 'exp_avg_sq: negative', lambda c: c['optimizer']['exp_avg_sq'][_first(c, 'exp_avg_sq')].view(-1)[0].fill_(-1e-3)),
    ('negative step', '^step:', lambda c: _set(c['optimizer'], 'step', -1)),
]


@pytest.fixture(scope='module')
def written(tmp_path_factory):
    d = tmp_path_factory.mktemp('ckpt')
    mp = pytest.MonkeyPatch()
    try:
        a = _trained(d, mp)
    finally:
        mp.undo()
    a.save_checkpoint(d / 'a.ckpt')
    a.save(str(d))
    return d, a


@pytest.mark.parametrize('initiated', [False, True])
@pytest.mark.parametrize('what,match,edit', EDITS, ids=[e[0] for e in EDITS])
def test_refusals_name_the_field_and_change_nothing(written, tmp_path, monkeypatch, what, match, edit, initiated):
    d, a = written
    monkeypatch.chdir(tmp_path)
    bad = _edit(d / 'a.ckpt', tmp_path / 'bad.ckpt', edit)
    b = _predictor(seed=31)
    if initiated:
        b.initiate_training(lr=0.02, lr_decay=0.9)
        _step(b, 50)
        b.train_loss, b.test_loss = [1.0], [2.0]
    before, rng = _snapshot(b), torch.get_rng_state()
    with pytest.raises(ValueError, match=match):
        b.load_checkpoint(bad)
    assert _same(before, _snapshot(b)) and torch.equal(rng, torch.get_rng_state()), what
    b.load_checkpoint(d / 'a.ckpt')         # (and the unedited file still loads into the same predictor)
    assert all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))


def test_a_weights_file_is_no_checkpoint(written, tmp_path, monkeypatch):
    d, a = written
    monkeypatch.chdir(tmp_path)
    b = _predictor(seed=31)
    before = _snapshot(b)
    with pytest.raises(ValueError, match='^format:'):
        b.load_checkpoint(d / f'{a.experiment_name}.pth')
    assert _same(before, _snapshot(b))


@pytest.mark.parametrize('kw,match', [(dict(conv='GCNConv'), "convolution_type='ChebConv' in the file, 'GCNConv' here"),
                                      (dict(hidden=16), 'hidden_size=8 in the file, 16 here'),
                                      (dict(binary=True), 'binary=False in the file, True here'),
                                      (dict(input_features=2), 'input_features=1 in the file, 2 here'),
                                      (dict(input_timesteps=4), 'input_timesteps=3 in the file, 4 here')])
def test_another_predictor_refuses_the_file(written, tmp_path, monkeypatch, kw, match):
    d, _ = written
    monkeypatch.chdir(tmp_path)
    b = _predictor(seed=31, **kw)
    before = _snapshot(b)
    with pytest.raises(ValueError, match=match):
        b.load_checkpoint(d / 'a.ckpt')
    assert _same(before, _snapshot(b)) and not b.training_initiated


def test_save_needs_a_training_state(tmp_path):
    with pytest.raises(ValueError, match='save_checkpoint'):
        _predictor().save_checkpoint(tmp_path / 'x.ckpt')
    assert os.listdir(tmp_path) == []


def test_flat_and_per_name_layouts():
    """qtmpnn.flat.split_flat / join_flat on a hand-made vector: flat -> per name -> flat is exact, and the pad tail behind the
    last parameter is neither stored nor written."""
    from qtmpnn.flat import join_flat, name_table, split_flat
    table = [('a.weight', 0, (2, 3)), ('a.bias', 6, (3,)), ('b', 9, ()), ('c.weight', 10, (1, 2, 2))]
    n, pad = 14, 4
    vec = torch.zeros(n + pad)
    vec[:n] = torch.arange(1, n + 1, dtype=torch.float32) * 0.37
    named = split_flat(vec, table)
    assert list(named) == [t[0] for t in table] and all(tuple(named[k].shape) == s for k, _, s in table)
    assert torch.equal(named['a.weight'], vec[:6].view(2, 3)) and torch.equal(named['b'], vec[9]) and named['b'].dim() == 0
    assert sum(v.numel() for v in named.values()) == n
    named['a.bias'] += 0                     # (copies: writing them does not write the vector)
    assert named['a.bias'].data_ptr() != vec[6:].data_ptr()
    out = torch.full((n + pad,), 7.0)
    out[n:] = 0
    ptr = out.data_ptr()
    assert join_flat(named, table, out) is out and out.data_ptr() == ptr
    assert torch.equal(out, vec) and bool((out[n:] == 0).all())
    tail = torch.full((n + pad,), 7.0)      # the tail is not written at all, whatever it holds
    join_flat(named, table, tail)
    assert torch.equal(tail[:n], vec[:n]) and bool((tail[n:] == 7.0).all())
    with pytest.raises(ValueError, match='a.bias'):
        join_flat(dict(named, **{'a.bias': torch.zeros(4)}), table, out)
    # the table of a module is that of its named_parameters(), which is the order FlatParams lays the buffer out in
    lin = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    assert name_table(lin) == [('0.weight', 0, (2, 3)), ('0.bias', 6, (2,)), ('1.weight', 8, (1, 2)), ('1.bias', 10, (1,))]


def test_adam_state_layout_is_shared_by_both_optimisers():
    """adam_state of torch's Adam, checked and loaded back into a second Adam: the per-name layout a FlatAdam reads and writes
    through name_table (the flat side of it runs on the GPU, tests/test_gpu_checkpoint.py)."""
    from qtmpnn.flat import name_table
    from qtmpnn.optim import adam_state, check_adam_state, load_adam_state
    torch.manual_seed(2)
    m1, m2 = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    o1, o2 = torch.optim.Adam(m1.parameters(), lr=0.1), torch.optim.Adam(m2.parameters(), lr=0.3)
    empty = adam_state(o1, m1)
    assert empty['step'] == 0 and all(not v.any() for v in empty['exp_avg'].values())
    for _ in range(2):
        m1(torch.ones(3)).sum().backward()
        o1.step()
    st = adam_state(o1, m1)
    check_adam_state(st, name_table(m2))
    load_adam_state(o2, m2, st)
    assert adam_state(o2, m2)['step'] == 2 and o2.param_groups[0]['lr'] == 0.1
    for k in ('exp_avg', 'exp_avg_sq'):
        assert all(torch.equal(adam_state(o2, m2)[k][n], st[k][n]) for n in st[k])
    m1.bias.grad = None                      # a parameter that skips a step: no single step count any more
    o1.step()
    with pytest.raises(ValueError, match='step'):
        adam_state(o1, m1)


def test_atomic_write(tmp_path, monkeypatch):
    a = _trained(tmp_path, monkeypatch)
    path = tmp_path / 'a.ckpt'
    a.save_checkpoint(path)
    good = path.read_bytes()
    _step(a, 10)
    real = torch.save

    def failing(obj, f, *args, **kw):
        real({'half': 1}, f)                 # something reaches the disk, then the write dies
        raise OSError('disk full')
    monkeypatch.setattr(torch, 'save', failing)
    with pytest.raises(OSError, match='disk full'):
        a.save_checkpoint(path)
    monkeypatch.setattr(torch, 'save', real)
    assert path.read_bytes() == good and [f for f in os.listdir(tmp_path) if f != 'runs'] == ['a.ckpt']
    seen = []
    monkeypatch.setattr(torch, 'save', lambda obj, f, *args, **kw: (seen.append(os.fspath(f)), real(obj, f))[1])
    a.save_checkpoint(path)
    assert len(seen) == 1 and seen[0] != os.fspath(path) and os.path.dirname(seen[0]) == str(tmp_path)
    assert path.read_bytes() != good and not os.path.exists(seen[0])
    b = _predictor(seed=3)
    b.load_checkpoint(path)
    assert _same(_snapshot(a), _snapshot(b))
