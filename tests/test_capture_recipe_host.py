"""The capture recipe of the graphed steps, host side: the pieces make_graphed_step, _graphed_accumulation and _graphed_inference
share -- the tile watch's every-64 rule, the static batch and its shapes, the flat gradient, capture on first sight of a shape."""
import pytest
import torch


@pytest.fixture
def tile_checks(monkeypatch):
    """check_tile_errors as model.mpnnlstm calls it, replaced by a recorder of its `always` arguments."""
    import model.mpnnlstm as M
    calls = []
    monkeypatch.setattr(M, 'check_tile_errors', lambda always=False: calls.append(always))
    return calls


@pytest.mark.parametrize('offset', [0, 62, 63])
@pytest.mark.parametrize('advance', [1, 2, 3, 64])
def test_tile_watch_checks_when_the_count_crosses_a_multiple_of_64(monkeypatch, tile_checks, advance, offset):
    from model.mpnnlstm import TileWatch
    from qtmpnn import mesh
    monkeypatch.setattr(mesh, '_TILE_USED', {'cuda:0'})
    watch = TileWatch()
    assert watch.uses_tiles and tile_checks == [True]             # the check after the capture
    if offset:
        watch.advance(offset)
    assert watch.replays == offset
    del tile_checks[:]
    count = offset
    for _ in range(200):
        before, count = count, count + advance
        watch.advance(advance)
        crossed = any(m % 64 == 0 for m in range(before + 1, count + 1))
        assert tile_checks == ([True] if crossed else []), (before, count)
        if advance == 1:
            assert crossed == (count % 64 == 0)
        del tile_checks[:]
    assert watch.replays == count
    watch.check()
    assert tile_checks == [True]


def test_tile_watch_without_tile_launches_never_reads_the_device_again(monkeypatch, tile_checks):
    from model.mpnnlstm import TileWatch
    from qtmpnn import mesh
    monkeypatch.setattr(mesh, '_TILE_USED', set())
    watch = TileWatch()
    assert not watch.uses_tiles and tile_checks == [False]
    for j in (1, 63, 64, 200):
        watch.advance(j)
    watch.check()
    assert tile_checks == [False, False] and watch.replays == 328


def test_static_batch_shapes_and_load():
    from model.mpnnlstm import StaticBatch, batch_shapes
    x, y, c = torch.rand(2, 3, 4, 4, 1), torch.rand(2, 5, 4, 4, 1), torch.rand(2, 5, 4, 4, 1)
    # the key train(use_graph=True) computed for a batch, with and without a climatology
    assert batch_shapes((x, y, None)) == (tuple(x.shape), tuple(y.shape), None)
    assert batch_shapes((x, y, c)) == (tuple(x.shape), tuple(y.shape), tuple(c.shape))
    assert batch_shapes((x, c)) == (tuple(x.shape), tuple(c.shape))              # (an inference batch that does not read y)
    full = StaticBatch(x, y, c)
    assert full.shapes == batch_shapes((x, y, c))
    ptrs = [t.data_ptr() for t in full.tensors]
    assert all(torch.equal(s, t) and s.data_ptr() != t.data_ptr() for s, t in zip(full.tensors, (x, y, c)))
    full.load(2 * x, 3 * y, 4 * c)
    assert all(torch.equal(s, t) for s, t in zip(full.tensors, (2 * x, 3 * y, 4 * c)))
    assert [t.data_ptr() for t in full.tensors] == ptrs                          # in place: the graphs hold these pointers
    # what the three captures' copy-in accepted before: no climatology; one given where none was captured (not read); no y
    bare = StaticBatch(x, y, None)
    assert bare.shapes == batch_shapes((x, y, None)) and bare.tensors[2] is None
    bare.load(2 * x, 3 * y)
    bare.load(4 * x, 5 * y, None)
    bare.load(6 * x, 7 * y, c)
    assert torch.equal(bare.tensors[0], 6 * x) and torch.equal(bare.tensors[1], 7 * y)
    rollout = StaticBatch(x, None, c)
    rollout.load(2 * x, None, 3 * c)
    assert rollout.tensors[1] is None and torch.equal(rollout.tensors[0], 2 * x) and torch.equal(rollout.tensors[2], 3 * c)
    # a captured shape that gets nothing to copy is an error, as it was
    with pytest.raises(TypeError):
        full.load(x, y)


def test_flat_gradient_is_the_vector_itself_or_a_concatenation_with_zeros():
    from qtmpnn.flat import FlatParams
    module = torch.nn.Linear(3, 2)
    fp = FlatParams(module)
    assert len(fp.params) == 2 and fp.n == 8
    g = torch.arange(8.0)
    fp.set_grad_vector(g)
    out = fp.gradient()
    assert out.data_ptr() == fp.last_grad.data_ptr() == g.data_ptr() and out.numel() == fp.n and torch.equal(out, g)
    # gradients that are no views of one vector: by copy, a parameter without a gradient counts as zero
    fp.zero_grad()
    module.weight.grad = torch.full((2, 3), 2.0)
    out = fp.gradient()
    assert fp.grad_vector() is None and module.bias.grad is None
    assert torch.equal(out, torch.tensor([2.0] * 6 + [0.0] * 2)) and out.data_ptr() != module.weight.grad.data_ptr()
    fp.zero_grad()
    assert torch.equal(fp.gradient(), torch.zeros(8))


def test_a_shape_is_captured_on_first_sight_and_replayed_after():
    from model.mpnnlstm import NextFramePredictorS2S
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=3, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))
    graphed, captures, replays = {}, [], []

    def capture(tag):
        captures.append(tag)
        nfp.last_warmup_loss = f'warm-up {tag}'
        return lambda *args: replays.append((tag, args)) or f'replay {tag}'
    a, b = (torch.zeros(2, 4, 4, 1), torch.zeros(3, 4, 4, 1), None), (torch.zeros(2, 2, 4, 4, 1), torch.zeros(2, 3, 4, 4, 1), None)
    assert nfp._first_sight(graphed, a, lambda: capture('a'), a) == 'warm-up a'
    assert nfp._first_sight(graphed, a, lambda: capture('a again'), a) == 'replay a'
    assert nfp._first_sight(graphed, b, lambda: capture('b'), ([b, b],)) == 'warm-up b'
    assert nfp._first_sight(graphed, b, lambda: capture('b again'), ([b, b],)) == 'replay b'
    assert captures == ['a', 'b'] and replays == [('a', a), ('b', ([b, b],))] and len(graphed) == 2


def test_fused_is_refused_before_any_launch(monkeypatch):
    from model.mpnnlstm import NextFramePredictorS2S
    from model.seq2seq import Seq2Seq
    nfp = NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=3, device=None,
                                model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1))

    def launched(*a, **k):
        raise AssertionError('a launch was reached before the refusal')
    monkeypatch.setattr(Seq2Seq, 'forward', launched)
    x, y = torch.zeros(2, 64, 64, 1), torch.zeros(3, 64, 64, 1)
    for call in (lambda: nfp.forward_loss(x, y, fused=True), lambda: nfp.accumulate_gradients([(x, y)], fused=True)):
        with pytest.raises(ValueError, match='fused: fused=True selects the fused binary cross-entropy and needs a binary=True'):
            call()
