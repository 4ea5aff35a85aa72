"""set_recompute('stream'), host side: the third value of the switch, its refusals (by name, before anything reaches a device), and
the bookkeeping of a streaming ops.GradAcc on plain CPU tensors -- no use of a packed weight keeps its weight-gradient operands
past its own backward, the sum is emitted once, by the first forward use, and the default keeps them as before."""
import pytest
import torch

T_ = 3
MODES = (None, 'step', 'stream')


def _predictor(**kw):
    from model.mpnnlstm import NextFramePredictorS2S
    return NextFramePredictorS2S(thresh=0.1, input_features=1, input_timesteps=2, output_timesteps=T_, device=None,
                                 model_kwargs=dict(hidden_size=8, dropout=0.0, n_layers=1), **kw)


def test_stream_is_a_mode_and_round_trips():
    from qtmpnn import recompute
    assert 'stream' in recompute.MODES and recompute.check_mode('stream') == 'stream'
    nfp = _predictor()
    assert nfp.recompute is None
    nfp.set_recompute('stream')
    assert nfp.recompute == 'stream' and nfp.model.recompute == 'stream'
    nfp.set_recompute('step')
    assert nfp.recompute == 'step'
    nfp.set_recompute(None)
    assert nfp.recompute is None and nfp.model.recompute is None


def test_recomputing_nests_and_restores_the_mode():
    nfp = _predictor()
    with nfp.recomputing('stream') as inside:
        assert inside is nfp and nfp.recompute == 'stream'
        with nfp.recomputing('step'):
            assert nfp.recompute == 'step'
            with nfp.recomputing(None):
                assert nfp.recompute is None
            assert nfp.recompute == 'step'
        assert nfp.recompute == 'stream'
    assert nfp.recompute is None
    nfp.set_recompute('stream')
    with pytest.raises(KeyError):
        with nfp.recomputing('step'):
            assert nfp.recompute == 'step'
            raise KeyError('x')
    assert nfp.recompute == 'stream'


@pytest.mark.parametrize('bad', ['steps', True, 1, 'Step', 0, False])
def test_other_values_are_still_refused_by_name(bad):
    nfp = _predictor()
    nfp.set_recompute('stream')
    with pytest.raises(ValueError, match='set_recompute'):
        nfp.set_recompute(bad)
    with pytest.raises(ValueError, match='set_recompute'):
        with nfp.recomputing(bad):
            raise AssertionError('the block ran')
    assert nfp.recompute == 'stream'


def test_description_does_not_know_the_mode():
    nfp = _predictor()
    seen = []
    for mode in MODES:
        nfp.set_recompute(mode)
        seen.append(nfp._description())
    assert seen[0] == seen[1] == seen[2] and 'recompute' not in str(seen[0]) and 'stream' not in str(seen[0])


def test_remesh_input_is_refused_before_any_launch(monkeypatch):
    from qtmpnn import _lib

    def launched(*a, **k):
        raise AssertionError('a launch was reached before the refusal')
    monkeypatch.setattr(_lib, 'call', launched)
    nfp = _predictor(remesh_input=True)
    nfp.set_recompute('stream')                                     # the switch itself is no refusal
    x = torch.zeros(3, 64, 64, 1)
    with pytest.raises(NotImplementedError, match=r"set_recompute\('stream'\).*remesh_input=True"):
        nfp.model.process_inputs(x)
    with pytest.raises(NotImplementedError, match=r"set_recompute\('stream'\)"):
        nfp.model(x, None)
    with torch.no_grad(), pytest.raises(RuntimeError, match='must live on the GPU'):        # without autograd: a no-op
        nfp.model.process_inputs(x)


class _Use(torch.autograd.Function):
    """h' = h + x w: one use of the shared weight w, chained to the next by h.  Its weight gradient goes the way of the Chebyshev and
    attention backward in qtmpnn.ops: operands to GradAcc.keep, the sum out of GradAcc.flush by the use that leave() names."""

    @staticmethod
    def forward(ctx, h, x, w, acc, log):
        ctx.save_for_backward(x)
        ctx.acc, ctx.log, ctx.use_idx = acc, log, acc.enter()
        return h + x * w

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        acc = ctx.acc

        def reduce(uses):           # the stand-in of the grouped launch: all given uses in one float32 sum
            ctx.log['launches'].append(len(uses))
            return [torch.stack([(xi * gi).sum(0) for xi, gi in uses]).sum(0)]
        acc.keep((x, g), reduce)
        ctx.log['kept'].append(len(acc.pending))
        gw = None
        if acc.leave(ctx.use_idx):
            gw = acc.flush(reduce)[0]
            ctx.log['emitted'].append(ctx.use_idx)
        ctx.log['after'].append(len(acc.pending))
        return g, None, gw, None, None


def _chain(stream, n=5):
    from qtmpnn import ops
    torch.manual_seed(3)
    w = torch.randn(7, requires_grad=True)
    xs = torch.randn(n, 11, 7)
    acc = ops.GradAcc()
    if stream:
        acc.stream = True
    log = {'kept': [], 'after': [], 'emitted': [], 'launches': []}
    h = torch.zeros(11, 7)
    for t in range(n):
        h = _Use.apply(h, xs[t], w, acc, log)
    (h * torch.linspace(0.5, 1.5, 7)).sum().backward()
    want = (xs.double() * torch.linspace(0.5, 1.5, 7).double()).sum((0, 1))
    return w.grad, want, acc, log


def test_streaming_gradacc_keeps_no_operands():
    from qtmpnn import ops
    assert ops.GradAcc().stream is False                    # the default defers
    grad, want, acc, log = _chain(stream=True)
    assert log['kept'] == [0] * 5 and log['after'] == [0] * 5 and acc.pending == []
    assert log['launches'] == [1] * 5                       # one use per reduction, in backward order
    assert log['emitted'] == [0] and acc.total is None      # once, by use 0; nothing is left behind
    # 55 products per entry summed in fp32, in any order: |error| <= 55 eps max|sum of magnitudes|; 1e-5 relative is far above it
    torch.testing.assert_close(grad.double(), want, rtol=1e-5, atol=1e-5)


def test_default_gradacc_keeps_the_operands_until_the_last_backward():
    grad, want, acc, log = _chain(stream=False)
    assert log['kept'] == [1, 2, 3, 4, 5] and log['after'] == [1, 2, 3, 4, 0]     # 4 operand sets wait for the last one
    assert log['launches'] == [5] and log['emitted'] == [0] and acc.pending == [] and acc.total is None
    torch.testing.assert_close(grad.double(), want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('stream', [False, True])
def test_use_0_before_a_later_use_still_raises(stream):
    from qtmpnn import ops
    acc = ops.GradAcc()
    acc.stream = stream
    w = torch.ones(7, requires_grad=True)
    log = {'kept': [], 'after': [], 'emitted': [], 'launches': []}
    a = _Use.apply(torch.zeros(2, 7), torch.ones(2, 7), w, acc, log)       # use 0 and use 1 side by side: not chained
    b = _Use.apply(torch.zeros(2, 7), torch.ones(2, 7), w, acc, log)
    with pytest.raises(RuntimeError, match='first use of a packed weight ran its backward before a later use'):
        a.sum().backward()
    del b


def test_stream_accs_marks_every_accumulator_of_a_pack():
    from qtmpnn import ops, recompute

    @recompute.register_record
    class Rec:
        __slots__ = ('W', 'acc')

        def __init__(self, W, acc):
            self.W, self.acc = W, acc
    try:
        pack = ({'cell': [Rec(torch.ones(2), ops.GradAcc())], 'acc1': ops.GradAcc()}, None)
        assert recompute.stream_accs(pack) is pack
        assert pack[0]['cell'][0].acc.stream is True and pack[0]['acc1'].stream is True
    finally:
        recompute._RECORDS.remove(Rec)
