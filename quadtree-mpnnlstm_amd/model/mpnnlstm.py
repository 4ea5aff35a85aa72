"""Trainer facade of the reference's model/mpnnlstm.py (NextFramePredictorS2S) around the HIP rollout.

Same constructor / train / predict / save / load surface; the train step (mpnnlstm.py:229-257) is
`train_step` below and additionally accepts batches of clips and a torch.distributed process group
(one flat gradient all-reduce per step).  tensorboard is optional (absent -> no-op writer).
"""
import collections
import collections.abc
import contextlib
import datetime
import inspect
import math
import os
import time
from abc import ABC, abstractmethod

import numpy as np
import pandas as pd
import torch
from torch.optim.lr_scheduler import StepLR

from model.graph_functions import image_to_graph, unflatten, plot_contours
from model.seq2seq import Seq2Seq, check_concat_clips
from model.utils import add_positional_encoding, get_n_params, int_to_datetime, launch_day_index, output_day_indices
from qtmpnn import mesh as _mesh, ops
from qtmpnn.baselines import (check_references, default_references, forecast_sources, launch_frame, needs_launch_climatology,
                              reference_fields, reference_launches, spec_name)
from qtmpnn.dist import all_reduce_sum, allreduce_gradients
from qtmpnn.flat import flat_params, name_table
from qtmpnn.horizon import first_steps, resolve_schedule
from qtmpnn._lib import on_device
from qtmpnn.mesh import check_tile_errors, host_mask

CHECKPOINT_FORMAT = 2       # the newest save_checkpoint() writes (1 without averaged weights, 2 with); load_checkpoint() refuses a newer one

try:                                        # pragma: no cover - optional dependency
    from torch.utils.tensorboard import SummaryWriter
except Exception:                           # tensorboard is not installed in the build image
    class SummaryWriter:
        def __init__(self, *a, **k):
            pass

        def add_scalar(self, *a, **k):
            pass

        def flush(self):
            pass


class LossWeights:
    """The checked weights of the weighted training loss: `weights` (W, H), non-negative pixel weights (None: ones), and
    `lead_weights` (T_out,), non-negative weights of the output steps (None: ones).  Everything is checked here, on the host and
    before any launch -- shape, finite, non-negative, a positive sum (of the pixel weights over the pixels `mask` leaves) -- and
    each refusal is a ValueError that names the argument.  The sums of the divisor are float64 sums of the float32 values the
    kernels read.  to(device) uploads the two arrays once; chunk(steps) is the view of a truncated-BPTT chunk.
    `pos_weight` (binary predictors only; None: 1) is the positive-class weight of masked_bce, carried beside the two arrays so
    that one object holds everything a trainer method was given; it is checked like them and does not enter the divisor."""

    def __init__(self, weights, lead_weights, shape, T_out, mask=None, pos_weight=None):
        shape, self.T = tuple(int(v) for v in shape), int(T_out)
        self.pos_weight = 1.0 if pos_weight is None else ops.check_pos_weight(pos_weight)
        mask = host_mask(mask)
        if mask is not None and tuple(mask.shape) != shape:
            raise ValueError(f'mask: shape {tuple(mask.shape)} for frames of {shape}')

        def host(a, name, want):
            if a is None:
                return np.ones(want, np.float32)
            a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
            if a.dtype == object or a.dtype.kind not in 'fiub':
                raise ValueError(f'{name}: a numeric array is needed, got dtype {a.dtype}')
            if tuple(a.shape) != want:
                raise ValueError(f'{name}: shape {tuple(a.shape)}, expected {want}')
            a = np.ascontiguousarray(a, dtype=np.float32)
            if not np.isfinite(a).all():
                raise ValueError(f'{name}: NaN or infinite entries')
            if (a < 0).any():
                raise ValueError(f'{name}: negative entries')
            return a
        self.w_host = host(weights, 'loss_weights', shape)
        self.lam_host = host(lead_weights, 'lead_weights', (self.T,))
        self.sum_w = float(self.w_host.astype(np.float64)[slice(None) if mask is None else ~mask].sum())
        self.sum_lam = float(self.lam_host.astype(np.float64).sum())
        if not self.sum_w > 0:
            raise ValueError('loss_weights: the weights of the unmasked pixels sum to 0')
        if not self.sum_lam > 0:
            raise ValueError('lead_weights: the weights sum to 0')
        self.shape, self.w, self.lam = shape, None, None

    def to(self, device):
        device = torch.device(device)
        if self.w is None or self.w.device.type != device.type or device.index not in (None, self.w.device.index):
            self.w = torch.from_numpy(self.w_host).reshape(-1).to(device)
            self.lam = torch.from_numpy(self.lam_host).to(device)
        return self

    def chunk(self, steps):
        """The weights of the output steps range `steps`: the same pixel weights, lead_weights[steps] and their own sum."""
        c = object.__new__(LossWeights)
        c.__dict__.update(self.__dict__)
        c.T = len(steps)
        c.lam_host = self.lam_host[steps.start:steps.stop]
        c.sum_lam = float(c.lam_host.astype(np.float64).sum())
        if not c.sum_lam > 0:
            raise ValueError(f'lead_weights: the weights of the truncated chunk of steps [{steps.start}, {steps.stop}) sum to 0')
        c.lam = None if self.lam is None else self.lam[steps.start:steps.stop]
        return c


def horizon_weights(lw, k):
    """The LossWeights `lw` (None: unweighted, and None comes back) cut to a horizon of k steps: the same pixel weights, the first
    k lead weights and the divisor those entries give (LossWeights.chunk) -- what train(horizon=) trains epoch by epoch with.
    Refused under `horizon`, on the host: k above the entries there are, and first entries that sum to 0."""
    if lw is None or k == lw.T:
        return lw
    if k > lw.T:
        raise ValueError(f'horizon: lead_weights has {lw.T} entries (the built output steps), horizon={k} needs {k}')
    if not float(lw.lam_host[:k].astype(np.float64).sum()) > 0:
        raise ValueError(f'horizon: the first {k} lead_weights sum to 0: horizon={k} would train on no step')
    return lw.chunk(range(k))


def loss_weights_of(weights, lead_weights, shape, T_out, mask=None, binary=False):
    """None when neither weight is given (the unweighted loss, untouched), a LossWeights as it is, else the checked pair."""
    if weights is None and lead_weights is None:
        return None
    if binary:
        raise ValueError('loss_weights / lead_weights: the weighted loss of masked_mse is the squared error; binary=True (BCE) takes '
                         'no weights here: the weighted binary cross-entropy is masked_bce')
    return _checked_weights(weights, lead_weights, shape, T_out, mask)


def _checked_weights(weights, lead_weights, shape, T_out, mask=None, pos_weight=None):
    """A LossWeights as it is (held to the frame shape and step count; with pos_weight given, a copy that carries it), else the
    checked weights, a missing array being ones."""
    if isinstance(weights, LossWeights):
        if lead_weights is not None:
            raise ValueError('lead_weights: already part of the LossWeights passed as the pixel weights')
        if weights.shape != tuple(shape) or weights.T != T_out:
            raise ValueError(f'loss_weights: prepared for {weights.T} steps of {weights.shape} frames, not {T_out} of {tuple(shape)}')
        if pos_weight is not None:
            pos_weight, lw = ops.check_pos_weight(pos_weight), weights
            weights = object.__new__(LossWeights)
            weights.__dict__.update(lw.__dict__)
            weights.pos_weight = pos_weight
        return weights
    return LossWeights(weights, lead_weights, shape, T_out, mask, pos_weight)


def bce_weights_of(weights, lead_weights, pos_weight, shape, T_out, mask=None):
    """The loss of a binary=True predictor: None when no weight of any kind is given (the unweighted BCE paths, untouched), else the
    checked LossWeights of masked_bce with its pos_weight (a missing array is ones, a missing pos_weight 1)."""
    if weights is None and lead_weights is None and pos_weight is None:
        return None
    return _checked_weights(weights, lead_weights, shape, T_out, mask, pos_weight)


def _rollout_targets(outputs, meshes, y):
    """y as (B, T_out, W, H, 1), refused unless it is the targets of this rollout."""
    if y.dim() == 4:
        y = y.unsqueeze(0)
    mesh0 = meshes[0]
    want = (mesh0.B, len(outputs), mesh0.n, mesh0.m, 1)
    if tuple(y.shape) != want:      # (the loss kernels read B x P targets per step straight from this buffer)
        raise ValueError(f'targets of shape {tuple(y.shape)} for {mesh0.B} clip(s) x {len(outputs)} output steps of {mesh0.n} x {mesh0.m} '
                         f'frames: expected (T_out, W, H, 1) or (B, T_out, W, H, 1) = {want}')
    return y


def _summed_loss(outputs, meshes, y, divisor, rollout, step, lw=None, *tail):
    """The sum of a rollout's loss terms / divisor, in one reduction for all steps.  rollout: ops.rollout_*_partials, all steps in
    one launch per kernel; where it returns None (loss_mask meshes, odd layouts) step: ops.step_*_partials, step by step,
    composed.  lw: the LossWeights of the weighted losses; tail: what follows the weights (pos_weight)."""
    y = y.to(outputs[0].device)
    w, lam = (lw.to(y.device).w, lw.lam) if lw is not None else (None, None)
    part = rollout(outputs, y, meshes, *(() if lw is None else (w, lam)), *tail)
    if part is None:
        part = torch.cat([step(out, y[:, t], mesh, *(() if lw is None else (w, lam[t])), *tail)
                          for t, (out, mesh) in enumerate(zip(outputs, meshes))])
    return part.sum() / float(divisor)


def masked_mse(outputs, meshes, y, mask=None, binary=False, weights=None, lead_weights=None, fused=False):
    """MSELoss(y_hat[:, ~mask], y[:, ~mask]) of mpnnlstm.py:243-246 without building y_hat:
    sum over steps of the per-mesh squared error, divided by (clips x steps x unmasked pixels).
    y: (T_out, W, H, 1) or (B, T_out, W, H, 1).

    Beyond the reference: weights (W, H) >= 0 and / or lead_weights (T_out,) >= 0 (a missing one is ones; or one LossWeights as
    `weights`) give  sum lam_t w_p d^2 / (B sum_t lam_t sum_{p unmasked} w_p)  over the same counted pixels, the divisor formed
    on the host in float64.  Unit weights are the unweighted loss; with neither given nothing here changes.

    binary=True is the reference's BCELoss on the sigmoid output.  As it stands it builds the (B, T, W, H, 1) frames and calls
    torch (a host-side boolean index: not capturable).  fused=True (binary only) takes the rollout launches instead
    (ops.rollout_bce_partials: no frames, no host read, the same bits on every run) and divides by B * T_out * unmasked pixels,
    the divisor of torch's mean; it is what a captured step runs."""
    if fused and not binary:
        raise ValueError('fused: fused=True selects the fused binary cross-entropy and needs binary=True (the squared error always '
                         'runs through the rollout launches)')
    y = _rollout_targets(outputs, meshes, y)
    mesh0 = meshes[0]
    lw = loss_weights_of(weights, lead_weights, (mesh0.n, mesh0.m), len(outputs), mask, binary)
    if lw is not None:
        return _summed_loss(outputs, meshes, y, mesh0.B * lw.sum_lam * lw.sum_w, ops.rollout_wsse_partials, ops.step_wsse_partials, lw)
    mask = host_mask(mask)
    n_valid = mesh0.P if mask is None else int((~mask).sum())
    if binary and not fused:
        y_hat = torch.stack([unflatten(o, ms, (ms.n, ms.m)).reshape(ms.B, ms.n, ms.m, 1) for o, ms in zip(outputs, meshes)], 1)
        keep = torch.ones(mesh0.n, mesh0.m, dtype=torch.bool) if mask is None else ~torch.as_tensor(mask)
        return torch.nn.functional.binary_cross_entropy(y_hat[:, :, keep], y.to(y_hat.device)[:, :, keep])
    loss = (ops.rollout_bce_partials, ops.step_bce_partials) if binary else (ops.rollout_sse_partials, ops.step_sse_partials)
    return _summed_loss(outputs, meshes, y, mesh0.B * len(outputs) * n_valid, *loss)


def masked_bce(outputs, meshes, y, mask=None, weights=None, lead_weights=None, pos_weight=1.0):
    """The weighted binary cross-entropy of a binary=True rollout (beyond the reference): over the pixels masked_mse counts,

        term(b, t, p) = -(pos_weight y L1 + (1 - y) L0),  L1 = max(log o, -100),  L0 = max(log(1 - o), -100)   (torch's clamp)
        loss          = sum lam_t w_p term / (B sum_t lam_t sum_{p unmasked} w_p)

    weights (W, H) >= 0 and lead_weights (T_out,) >= 0 as in masked_mse (a missing one is ones; or one LossWeights as `weights`),
    the divisor formed on the host in float64; pos_weight, one finite number > 0, weighs the y = 1 side and does not enter the
    divisor (the convention of torch's BCEWithLogitsLoss(pos_weight=)).  Unit weights and pos_weight = 1 are
    masked_mse(binary=True, fused=True).  Always the rollout launches (ops.rollout_wbce_partials; ops.step_wbce_partials for
    loss_mask meshes and odd layouts): no frames, no host read, capturable, the same bits on every run.  Every refusal is a
    ValueError that names the argument, before any launch."""
    y = _rollout_targets(outputs, meshes, y)
    mesh0 = meshes[0]
    lw = _checked_weights(weights, lead_weights, (mesh0.n, mesh0.m), len(outputs), mask)
    pos_weight = ops.check_pos_weight(pos_weight)
    return _summed_loss(outputs, meshes, y, mesh0.B * lw.sum_lam * lw.sum_w, ops.rollout_wbce_partials, ops.step_wbce_partials, lw,
                        pos_weight)


def weighted_loss(y_hat, meshes, y, mask, lw, binary):
    """The weighted loss of a head, lw its LossWeights: masked_bce on a binary=True one, else masked_mse."""
    if binary:
        return masked_bce(y_hat, meshes, y, mask, weights=lw, pos_weight=lw.pos_weight)
    return masked_mse(y_hat, meshes, y, mask, weights=lw)


# -- gradient accumulation: one optimiser step from k micro-batches (beyond the reference) -------------------------------------
def check_accumulate(accumulate):
    """accumulate as an integer >= 1, or a ValueError that names it."""
    if isinstance(accumulate, bool) or not isinstance(accumulate, (int, np.integer)) or accumulate < 1:
        raise ValueError(f'accumulate: an integer >= 1 is needed (the micro-batches of one optimiser step), got {accumulate!r}')
    return int(accumulate)


def micro_weights(clips):
    """The weights of the micro-batches of one accumulated step, w_i = B_i / sum_j B_j for micro-batches of B_i clips: every
    rollout loss divides by its own clip count (masked_mse, masked_bce: B x steps x pixels, or B x the weight sums), so these
    weights make sum_i w_i L_i the loss, and sum_i w_i grad_i the gradient, of the concatenated batch."""
    clips = [int(b) for b in clips]
    if not clips or min(clips) < 1:
        raise ValueError(f'batches: every micro-batch needs at least one clip, got the clip counts {clips}')
    total = sum(clips)
    return [b / total for b in clips]


def micro_multipliers(clips):
    """micro_weights as the accumulated step forms them: ([n_i], scale) with n_i = B_i / gcd(B), an integer, and scale =
    1 / sum_i n_i, so that w_i = n_i * scale.  The sum takes n_i * grad_i and is scaled ONCE at the end; micro-batches of one
    clip count give n_i = 1 and scale = group_scale(k), what the graphed step computes."""
    clips = [int(b) for b in clips]
    micro_weights(clips)                    # (refuses an empty list and a micro-batch without clips)
    g = math.gcd(*clips)
    return [b // g for b in clips], 1.0 / sum(b // g for b in clips)


def group_scale(j, world=1):
    """What a graphed accumulated step multiplies the sum of j micro-batch gradients (of one shape, summed over `world` ranks)
    by: 1 / (j * world).  A short last group of an epoch replays the same graphs with its own j."""
    if j < 1 or world < 1:
        raise ValueError(f'batches: a group of {j} micro-batch(es) over {world} rank(s)')
    return 1.0 / (j * world)


def checked_batches(who, batches):
    """`batches` of an accumulated step as a list of (x, y, concat_layers or None), or a ValueError under `who` that names what
    is wrong, on the host and before any launch: an empty sequence, an item that is no (x, y) or (x, y, concat_layers), frames
    of differing shapes, a concat_layers for some items and not for others."""
    if isinstance(batches, (torch.Tensor, np.ndarray)) or not isinstance(batches, collections.abc.Iterable):
        raise ValueError(f'{who}: batches must be a sequence of (x, y) or (x, y, concat_layers), got {type(batches).__name__}')
    items = []
    for i, item in enumerate(batches):
        if isinstance(item, (torch.Tensor, np.ndarray)) or not isinstance(item, collections.abc.Sequence) or len(item) not in (2, 3):
            raise ValueError(f'{who}: batches[{i}] must be (x, y) or (x, y, concat_layers)')
        items.append((item[0], item[1], item[2] if len(item) == 3 else None))
    if not items:
        raise ValueError(f'{who}: batches is empty: an optimiser step needs at least one micro-batch')
    clip = lambda t: tuple(t.shape[-4:])           # (T, W, H, C): everything but the clip count
    for i, (x, y, c) in enumerate(items):
        if x.dim() not in (4, 5) or y.dim() != x.dim():
            raise ValueError(f'{who}: batches[{i}]: x and y must both be (T, W, H, C) or both (B, T, W, H, C), got '
                             f'{tuple(x.shape)} and {tuple(y.shape)}')
        if clip(x) != clip(items[0][0]) or clip(y) != clip(items[0][1]):
            raise ValueError(f'{who}: batches[{i}] has another frame shape than batches[0]: x {tuple(x.shape)}, y {tuple(y.shape)} '
                             f'after x {tuple(items[0][0].shape)}, y {tuple(items[0][1].shape)} (only the clip count may differ)')
        if (c is None) != (items[0][2] is None):
            raise ValueError(f'{who}: concat_layers is given for some micro-batches and not for others (batches[{i}] '
                             f'{"has none" if c is None else "has one"}, batches[0] {"none" if items[0][2] is None else "one"})')
        check_concat_clips(x, c)
    return items


# -- the capture recipe: what make_graphed_step, _graphed_accumulation and _graphed_inference share -----------------------------
def batch_shapes(item):
    """The shapes of a batch (x, y, concat), None for a member that is None: what "the same batch shape" means to every cache of
    captured graphs and to a captured step that checks what it is given."""
    return tuple(None if t is None else tuple(t.shape) for t in item)


class StaticBatch:
    """Clones of a batch (x, y, concat, c0), any of which may be None, that captured graphs read their inputs from.  The graphs hold
    bare pointers: every buffer they read or write outside their own pools -- these clones, the loss weights, an accumulator -- has
    to live as long as whatever replays them, so a step object keeps them (its closure, step.loss_weights, step.buffers; a buffer
    named nowhere else is freed, the allocator hands its memory to the next tensor and a replay reads or adds into that)."""

    def __init__(self, x, y, concat, c0=None):
        """c0: the climatology of the launch-state day (get_launch_climatology), which travels with the batch as concat does
        where an anomaly-persistence reference is asked for; None otherwise, and then no member."""
        self.tensors = tuple(t if t is None else t.clone() for t in (x, y, concat) + (() if c0 is None else (c0,)))
        self.shapes = batch_shapes(self.tensors)

    def load(self, x, y, concat_layers=None, c0=None):
        """Copy a batch of the captured shapes in, x first; what has no clone here is not read."""
        for static, t in zip(self.tensors, (x, y, concat_layers, c0)):
            if static is not None:
                static.copy_(t)


def warm_then_sync(side, multi, fn):
    """Run the eager warm-up fn() and order it against the side stream that captures next -> fn()'s result."""
    if multi:
        # The warm-up steps all-reduce, and torch issues a synchronous collective -- and records its completion event -- on the
        # CURRENT stream.  The process group's watchdog thread polls that event (hipEventQuery) until the work is reaped, and
        # HIP refuses the query while the event's stream is capturing (hipErrorCapturedEvent: the watchdog dies and takes the
        # process with it; seen in round 5 as soon as RCCL was executed at all).  So under torch.distributed the warm-up runs
        # on the caller's stream and only the capture on the side stream: no collective ever touches a stream that captures.
        result = fn()
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
    else:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            result = fn()
        torch.cuda.current_stream().wait_stream(side)
    return result


class TileWatch:
    """The captured launches report failures (a tile-resident launch that gave up waiting) only through the device's persistent
    error word: it is read when this is made, after the capture, and then whenever advance() takes the replay count across a
    multiple of 64 -- one 4-byte copy, only for graphs that contain such launches at all."""

    def __init__(self):
        self.uses_tiles, self.replays = bool(_mesh._TILE_USED), 0
        self.check()

    def check(self):
        check_tile_errors(always=self.uses_tiles)

    def advance(self, j=1):
        before, self.replays = self.replays, self.replays + j
        if self.uses_tiles and before // 64 != self.replays // 64:
            check_tile_errors(always=True)


# The products of one inference rollout.  Each is reduce(y_hat, meshes, x, y, concat, named=None) -> one device tensor, written
# once: the eager branch of the inference loop and the captured body (NextFramePredictorS2S._graphed_product) call the same
# function.  None writes what another reads, so any of them may follow one rollout in any order (PRODUCTS, below the trainer).
# named: the product's reference forecasts for the batch, the ordered [(name, tensor)] that ops.with_references takes, made
# from the batch's fields (baselines.reference_fields: built once per batch for all products); None: the default ones.
def default_named(x, concat, persistence=True):
    """The default references of a batch as [(name, tensor)]: persistence (not for the event dates) and, with concat, climatology."""
    return ([('persistence', launch_frame(x))] if persistence else []) + ([('climatology', concat)] if concat is not None else [])


def reference_frames(image_shape, mask):
    """Frames by the reference's path (`unflatten` per step, in the caller's mode, one host copy per step): what an eager predict
    returns.  The only reduce whose result is a host array, (B, T_out, W, H, 1); it cannot be captured."""
    def reduce(y_hat, meshes, x, y, concat, named=None):
        frames = [unflatten(o, ms, image_shape, mask).cpu().numpy() for o, ms in zip(y_hat, meshes)]
        return np.stack(frames, axis=0)[None] if x.dim() == 4 else np.stack(frames, axis=1)
    return reduce


def frames_product(x, T_out):
    """Frames: every step gathered by one launch into its slot of a (B, T_out, W, H, 1) stack for batches shaped like x."""
    out = torch.empty(1 if x.dim() == 4 else x.shape[0], T_out, x.shape[-3], x.shape[-2], 1, device=x.device)

    def reduce(y_hat, meshes, x, y, concat, named=None):
        for t, (o, ms) in enumerate(zip(y_hat, meshes)):
            ops.gather_frame_into(o, ms, out, t)
        return out
    return reduce


def sums_product(threshold, maps=None):
    """Sums: the (T_out, B, S, 8) float64 verification sums of the model and the references `named` (None: persistence and, with
    concat, climatology); with `maps`, a float64 (T_out, S, 8, P) device buffer, the batch's per-pixel sums are added into it as
    well -- for more than two references a list of buffers, one per launch (maps_shapes): every launch adds into a block of
    its own, so that the model's sums are not added twice."""
    def reduce(y_hat, meshes, x, y, concat, named=None):
        named = default_named(x, concat) if named is None else named
        part = ops.with_references(lambda **slots: ops.rollout_scores(y_hat, meshes, y, threshold, **slots), named, 2)
        if maps is not None:           # (each launch adds into its block in place: nothing to collect, joined_maps reads them once)
            blocks = maps if isinstance(maps, (list, tuple)) else [maps]
            for block, (i, j) in zip(blocks, reference_launches(len(named)), strict=True):
                ops.rollout_score_maps(y_hat, meshes, y, block, threshold, **ops.reference_slots(named[i:j]))
        return part
    return reduce


def maps_blocks(T_out, k, P, device):
    """The zeroed maps buffers of k references: one float64 (T_out, 1 + n_i, 8, P) block per launch, n_i its references."""
    return [torch.zeros(T_out, 1 + j - i, 8, P, dtype=torch.float64, device=device) for i, j in reference_launches(k)]


def joined_maps(blocks):
    """(T_out, S, 8, P) of maps_blocks' buffers: the model's and the first launch's rows, then every other launch's own."""
    return blocks[0] if len(blocks) == 1 else torch.cat([blocks[0]] + [b[:, 1:] for b in blocks[1:]], dim=1)


def loss_product(mask, lw, binary, fused):
    """Loss: the rollout's training loss against y as a 0-d float32 device tensor -- what forward_loss computes after its
    forward, by the same rule: masked_mse(binary, fused) without weights (lw None), else the weighted loss of the head
    (weighted_loss).  The reduce of train()'s test pass; no row of PRODUCTS.  fused=True (binary heads) is the loss a capture can
    hold."""
    def reduce(y_hat, meshes, x, y, concat, named=None):
        if lw is None:
            return masked_mse(y_hat, meshes, y, mask, binary, fused=fused)
        return weighted_loss(y_hat, meshes, y, mask, lw, binary)
    return reduce


def reliability_product(threshold, bins):
    """Bin sums: the (T_out, B, S, K, 4) float64 probability verification sums of the model and the references (sums_product),
    K = bins (ops.rollout_reliability)."""
    def reduce(y_hat, meshes, x, y, concat, named=None):
        return ops.with_references(lambda **slots: ops.rollout_reliability(y_hat, meshes, y, threshold, bins, **slots),
                                   default_named(x, concat) if named is None else named, 2)
    return reduce


def fss_product(threshold, scales):
    """Neighbourhood sums: the (T_out, B, S, K, 5) int64 Fractions Skill Score sums of the model and the references
    (sums_product), K = len(scales) (ops.rollout_fss)."""
    def reduce(y_hat, meshes, x, y, concat, named=None):
        return ops.with_references(lambda **slots: ops.rollout_fss(y_hat, meshes, y, threshold, scales, **slots),
                                   default_named(x, concat) if named is None else named, 2)
    return reduce


def edge_product(threshold):
    """Ice-edge distance sums: the (T_out, B, S, 8) int64 sums of the model and the references (sums_product)
    (ops.rollout_edges)."""
    def reduce(y_hat, meshes, x, y, concat, named=None):
        return ops.with_references(lambda **slots: ops.rollout_edges(y_hat, meshes, y, threshold, **slots),
                                   default_named(x, concat) if named is None else named, 2)
    return reduce


def extent_product(threshold, region_dev, area_dev, R):
    """Regional extent sums: the (T_out, B, R, 1 + S, 4) float64 sums of the truth (row 0) and of the model and the references
    (sums_product) (ops.rollout_extent); region_dev / area_dev: the device maps of ops.rollout_extent, or None."""
    def reduce(y_hat, meshes, x, y, concat, named=None):
        return ops.with_references(lambda **slots: ops.rollout_extent(y_hat, meshes, y, threshold, region_dev, area_dev, R, **slots),
                                   default_named(x, concat) if named is None else named, 3, lead=2)
    return reduce


def _extent_maps(who, regions, areas, shape, device, region_names=None):
    """ops.check_regions, the names of the regions checked against R, and the two maps uploaded once -> (region_dev, area_dev,
    R, names)."""
    region, area, R = ops.check_regions(who, regions, areas, shape)
    names = tuple(f'region{r}' for r in range(R)) if region_names is None else tuple(region_names)
    if len(names) != R or len(set(names)) != R:
        raise ValueError(f'{who}: region_names must be {R} distinct names (the regions map has indices 0..{R - 1}), got {names}')
    up = lambda a: None if a is None else torch.from_numpy(a).to(device).view(-1)
    return up(region), up(area), R, names


def events_product(threshold, kind, persist):
    """Event buffer: int32, the int64 sums (B, S1 - 1, 8) followed by the dates (B, S1, P) (split_event_buffer) of observed,
    model and the references `named` (None: climatology, with concat; there is no persistence by default)."""
    def reduce(y_hat, meshes, x, y, concat, named=None):
        return ops.event_buffer(y_hat, meshes, y, launch_frame(x), threshold, kind, persist,
                                default_named(x, concat, persistence=False) if named is None else named)
    return reduce


def split_event_buffer(buf, B, S1, frame):
    """Host copy of ops.rollout_event_dates' buffer -> (dates (B, S1, W, H) int32, sums (B, S1 - 1, 8) int64)."""
    nsum = 2 * B * (S1 - 1) * 8
    return buf[nsum:].reshape(B, S1, *frame), buf[:nsum].view(np.int64).reshape(B, S1 - 1, 8)


# The product table: what each method of the inference loop is, stated once.  NextFramePredictorS2S.verify and the product's own
# method (predict, score, ...) both read it.
ProductCall = collections.namedtuple('ProductCall', 'T_out shape device with_clim graphed mask references', defaults=(None,))
ProductCall.__doc__ = """What a product is told about the call it is part of: the output steps, the frame shape (W, H) (None where a
loader does not say), the device, whether there is a climatology, whether the rollout is captured, the mask, and the call's
`references` (None: the default): as given where make_products gets it, checked (baselines.check_references) and, where
verify(products={name: dict(references=...)}) gives the product its own, replaced by those where a product gets it."""


class Product:
    """One product of the inference loop for one call; a row of PRODUCTS is its class.  Four entries:
        __init__(who, call, **options)   check and prepare, on the host and before any launch other than an upload: the checks
                                         of the method, refused under `who`; `options` are the method's keywords, all given
        reduce(x)                        make the reduce(y_hat, meshes, x, y, concat) for batches shaped like x
        collect(result, x)               take one batch's result to the host
        finish()                         the method's return value from what was collected
    and, where every batch needs something done before its rollout, begin(x).  reads_y: whether the reduce reads y.
    reset() forgets what was collected and keeps what was prepared: the same object then serves another pass over a loader,
    the captures made from its reduce included (train()'s test pass, once per epoch)."""
    reads_y, begin = True, None
    refs = None         # the reference specs of this product in the call, as make_products checked them; None: the default ones

    def named(self, fields):
        """This product's references for a batch, [(name, tensor)] from the batch's fields; None: the default ones."""
        return None if self.refs is None else [(spec_name(s), fields[s]) for s in self.refs]


class _Frames(Product):
    """predict: eagerly the reference's path, captured the gathered stack."""
    reads_y = False

    def __init__(self, who, call):
        self.graphed, self.T_out, self.preds = call.graphed, call.T_out, []
        if not call.graphed:
            if call.shape is None:
                raise AttributeError(f'{who}: the loader has no dataset.image_shape')
            self.reference = reference_frames(call.shape, call.mask)

    def reduce(self, x):
        return frames_product(x, self.T_out) if self.graphed else self.reference

    def collect(self, frames, x):
        self.preds.extend(frames.cpu().numpy() if self.graphed else frames)     # (the stack comes back with one host copy)

    def finish(self):
        return np.stack(self.preds, 0)

    def reset(self):
        self.preds = []


class _Sums(Product):
    """A product whose reduce leaves (T, B, ...) sums per batch: the loader's (B_total, T, ...) array, one host copy per batch."""

    def __init__(self, who, call, **options):
        self.refs = call.references
        self.sources, self.parts = forecast_sources(call.with_clim, self.refs), []
        self.prepare(who, call, **options)

    def reduce(self, x):
        return self.reducer

    def collect(self, part, x):
        self.parts.append(np.moveaxis(part.cpu().numpy(), 0, 1))

    def sums(self):
        return np.concatenate(self.parts, 0)

    def reset(self):
        self.parts = []


class _Scores(_Sums):
    maps = None

    def prepare(self, who, call, threshold):
        self.threshold = threshold

    def reduce(self, x):
        return sums_product(self.threshold, self.maps)

    def finish(self):
        from qtmpnn.score import Scores
        return Scores(self.sums(), self.sources)


class _ScoreMaps(_Scores):
    def prepare(self, who, call, threshold):
        self.who, self.threshold, self.T_out, self.frame = who, threshold, call.T_out, None

    def begin(self, x):         # the maps buffer exists, zeroed, before the first batch's forward; every batch has its grid
        if self.maps is None:
            self.frame = tuple(x.shape[-3:-1])
            blocks = maps_blocks(self.T_out, len(self.sources) - 1, self.frame[0] * self.frame[1], x.device)
            self.maps = blocks[0] if len(blocks) == 1 else blocks       # (more than two references: one block per launch)
        elif tuple(x.shape[-3:-1]) != self.frame:
            raise ValueError(f'{self.who}: a batch of {tuple(x.shape[-3:-1])} frames after {self.frame} ones: maps need '
                             'one grid (use one loader per grid)')

    def finish(self):
        from qtmpnn.score import ScoreMaps, Scores
        maps = self.maps
        if maps is not None:
            maps = joined_maps(maps if isinstance(maps, list) else [maps])
            maps = ScoreMaps(maps.cpu().numpy().reshape(*maps.shape[:3], *self.frame), self.sources)
        return Scores(self.sums(), self.sources, maps=maps)

    def reset(self):            # (the buffer is zeroed where it is: a capture made for this product adds into it by pointer)
        self.parts = []
        for block in (self.maps if isinstance(self.maps, list) else [] if self.maps is None else [self.maps]):
            block.zero_()


class _Reliability(_Sums):
    def prepare(self, who, call, threshold, bins):
        ops.check_bins(who, bins)
        self.threshold, self.reducer = threshold, reliability_product(threshold, bins)

    def finish(self):
        from qtmpnn.reliability import Reliability
        return Reliability(self.sums(), self.sources, self.threshold)                  # (B, T, S, K, 4)


class _FSS(_Sums):
    def prepare(self, who, call, threshold, scales):
        self.threshold, self.scales = threshold, ops.check_scales(who, scales)
        self.reducer = fss_product(threshold, self.scales)

    def finish(self):
        from qtmpnn.fss import FSS
        return FSS(self.sums(), self.sources, self.threshold, self.scales)             # (B, T, S, K, 5)


class _Edges(_Sums):
    def prepare(self, who, call, threshold):
        self.threshold, self.reducer = threshold, edge_product(threshold)

    def finish(self):
        from qtmpnn.edges import EdgeDistance
        return EdgeDistance(self.sums(), self.sources, self.threshold)                 # (B, T, S, 8)


class _Extent(_Sums):
    def prepare(self, who, call, threshold, regions, areas, region_names):
        if call.shape is None:
            raise AttributeError(f'{who}: the loader has no dataset.image_shape')
        region_dev, area_dev, R, self.names = _extent_maps(who, regions, areas, call.shape, call.device, region_names)
        self.threshold, self.reducer = threshold, extent_product(threshold, region_dev, area_dev, R)

    def finish(self):
        from qtmpnn.extent import Extent
        return Extent(self.sums(), self.sources, self.threshold, self.names)           # (B, T, R, 1 + S, 4)


class _Events(Product):
    def __init__(self, who, call, threshold, kind, persist):
        if kind not in ops.EVENT_KINDS:
            raise ValueError(f'{who}: kind must be one of {ops.EVENT_KINDS}, got {kind!r}')
        if not (isinstance(persist, int) and 1 <= persist <= call.T_out):
            raise ValueError(f'{who}: persist must be an integer in 1..{call.T_out} (the output steps), got {persist!r}')
        refs = self.refs = call.references             # (no persistence by default here)
        self.sources = ('observed',) + forecast_sources(call.with_clim, default_references(call.with_clim)[1:] if refs is None else refs)
        self.options, self.reducer = (kind, persist, threshold), events_product(threshold, kind, persist)
        self.dates, self.sums = [], []

    def reduce(self, x):
        return self.reducer

    def collect(self, buf, x):
        d, s = split_event_buffer(buf.cpu().numpy(), 1 if x.dim() == 4 else x.shape[0], len(self.sources), tuple(x.shape[-3:-1]))
        self.dates.append(d)
        self.sums.append(s)

    def finish(self):
        from qtmpnn.events import EventDates
        return EventDates(np.concatenate(self.dates, 0), np.concatenate(self.sums, 0), self.sources, *self.options)

    def reset(self):
        self.dates, self.sums = [], []


PRODUCTS = {'predict': _Frames, 'score': _Scores, 'score_maps': _ScoreMaps, 'reliability': _Reliability, 'fss': _FSS,
            'edge_distance': _Edges, 'extent': _Extent, 'event_dates': _Events}
DEFAULT_PRODUCTS = ('score', 'reliability', 'fss', 'edge_distance', 'extent', 'event_dates')


def product_options(name):
    """The keywords of product `name` and their defaults: the parameters of the method of that name that follow use_graph."""
    params = list(inspect.signature(getattr(NextFramePredictorS2S, name)).parameters.values())
    return {p.name: p.default for p in params[[p.name for p in params].index('use_graph') + 1:]}


def make_products(who, products, call):
    """`products` of a verify call -> {name: Product} in the order given, every one checked and prepared.  products: a sequence
    of names of PRODUCTS, or a mapping name -> dict of the product's keywords (None: none); a missing keyword takes the default
    of the product's method.  The refusals of the request itself are ValueErrors under `who` that name the product, and come
    before any product is looked at; a product's own checks then report under its method's name."""
    if isinstance(products, collections.abc.Mapping):
        asked = [(name, {} if options is None else options) for name, options in products.items()]
    elif isinstance(products, str) or not isinstance(products, collections.abc.Iterable):
        raise ValueError(f'{who}: products must be a sequence of product names or a mapping from a name to its keywords, got '
                         f'{products!r}')
    else:
        asked = [(name, {}) for name in products]
    if not asked:
        raise ValueError(f'{who}: products is empty: name at least one of {tuple(PRODUCTS)}')
    seen, known = set(), {}
    for name, options in asked:
        if not isinstance(name, str) or name not in PRODUCTS:
            raise ValueError(f'{who}: unknown product {name!r}: the products are {tuple(PRODUCTS)}')
        if name in seen:
            raise ValueError(f'{who}: product {name!r} is given twice: one configuration per product (make a second call for a '
                             'second one)')
        seen.add(name)
        known[name] = product_options(name)
        if not isinstance(options, collections.abc.Mapping):
            raise ValueError(f'{who}: the keywords of product {name!r} must be a dict, got {options!r}')
        for key in options:
            if key not in known[name] and (key != 'references' or name == 'predict'):
                raise ValueError(f'{who}: product {name!r} takes no keyword {key!r}: {name}() takes {tuple(known[name]) or "none"}')
    # the call's references are checked once and shared, so that every product reads the same fields; a product's own go first
    check = lambda who, refs: None if refs is None else check_references(who, refs, call.with_clim, call.T_out, call.shape)
    shared = check(who, call.references)
    made = {}
    for name, options in asked:
        options = dict(options)
        own = check(name, options.pop('references', None))
        made[name] = PRODUCTS[name](name, call._replace(references=shared if own is None else own), **{**known[name], **options})
    return made


def product_specs(products):
    """The distinct reference specs of some products, in order of first use: what one batch's fields are built for."""
    specs = []
    for p in products:
        specs += [s for s in (p.refs or ()) if not any(s is t or (isinstance(s, str) and s == t) for t in specs)]
    return tuple(specs)


def with_fields(products, reduces):
    """One reduce for several products of a rollout: every product's reduce on it, each with its own references from the
    batch's fields -> the tuple of their results."""
    pairs = list(zip(products, reduces))
    return lambda y_hat, meshes, x, y, concat, fields=None: tuple(
        reduce(y_hat, meshes, x, y, concat, p.named(fields)) for p, reduce in pairs)


def takes_references(method):
    """Gives a verification method of the predictor the keyword `references=None` (qtmpnn.baselines: a sequence of
    'persistence', 'climatology', 'anomaly_persistence' or AnomalyPersistence objects; None: persistence and, with a
    climatology, climatology, the call as it was) and a maker of a captured product (make_graphed_*), and only a maker, besides,
    `launch_climatology=None`: the given batch's climatology of the launch-state day (get_launch_climatology), which an anomaly reference reads and which
    then follows concat in the replay's arguments.  The parameter lists of these methods are read by the product table
    (product_options: what follows use_graph is a product's keywords) and stay as they are; what every one of them takes
    alike is taken here, in one place, and held in self._asked while the call runs -- _verify and the makers read it there.
    The specs are checked with the products (make_products), before the first batch and before any launch."""
    import functools
    maker = method.__name__.startswith('make_graphed_')

    @functools.wraps(method)
    def wrapper(self, *args, references=None, **keywords):
        launch_climatology = keywords.pop('launch_climatology', None) if maker else None       # (refused as unknown elsewhere)
        # every call sets its own, None included: a call made while another runs (a Monitor's value function, a callback)
        # does not inherit the outer call's references
        previous, self._asked = self._asked, (references, launch_climatology)
        try:
            return method(self, *args, **keywords)
        finally:
            self._asked = previous
    return wrapper


def takes_ema(method):
    """Gives train() the keywords `ema=None` and `ema_eval=True` (NextFramePredictorS2S.set_ema, averaged_weights).  train()'s
    parameter list is read by signature tests and stays as it is (takes_references); the two are taken and checked here, on
    the host and before anything else runs, and held in self._ema_asked = (decay or None, ema_eval) while the call runs.
    Refusals name the keyword: `ema` as set_ema refuses it; `ema_eval` a TypeError unless True or False, and a ValueError
    when it is given at all while no average is or becomes active (there is nothing to evaluate)."""
    import functools
    from qtmpnn import validation
    from qtmpnn.ema import check_decay

    @functools.wraps(method)
    def wrapper(self, *args, **keywords):
        given = 'ema_eval' in keywords
        ema, ema_eval = keywords.pop('ema', None), validation.check_flag('ema_eval', keywords.pop('ema_eval', True))
        decay = None if ema is None else check_decay(ema)
        if given and decay is None and self.ema is None:
            raise ValueError(f'ema_eval: ema_eval={ema_eval} without averaged weights: pass ema=decay (or call set_ema) first')
        previous, self._ema_asked = self._ema_asked, (decay, ema_eval)
        try:
            return method(self, *args, **keywords)
        finally:
            self._ema_asked = previous
    return wrapper


def takes_horizon(method):
    """Gives train() the keyword `horizon=None` (a horizon curriculum: qtmpnn.horizon.resolve_schedule has the three forms).
    train()'s parameter list is read by signature tests and stays as it is (takes_references, takes_ema); the keyword is taken
    here and held in self._horizon_asked while the call runs.  train() resolves and checks the whole schedule of its epochs
    before it makes the optimiser and before any launch."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *args, horizon=None, **keywords):
        previous, self._horizon_asked = self._horizon_asked, horizon
        try:
            return method(self, *args, **keywords)
        finally:
            self._horizon_asked = previous
    return wrapper


_NOT_GIVEN = object()       # train(trainable=) left out: the predictor's setting stays (None asks for all parameters)


def takes_trainable(method):
    """Gives train() the keyword `trainable` (NextFramePredictorS2S.set_trainable: None or a sequence of fnmatch patterns over
    the state-dict names).  train()'s parameter list is read by signature tests and stays as it is (takes_ema, takes_horizon);
    the keyword is taken here, checked and resolved against the model's names on the host, before anything else runs, and
    held in self._trainable_asked while the call runs.  train() applies it once the optimiser exists -- after
    initiate_training, which returns to all-trainable, when it has to make the optimiser itself -- and the setting that was
    in force before is back when the call ends, also after an exception.  Left out, the predictor's setting stays."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *args, trainable=_NOT_GIVEN, **keywords):
        if trainable is _NOT_GIVEN:
            return method(self, *args, **keywords)
        self._check_trainable(trainable)        # (every refusal of set_trainable but the one about the optimiser, which train() makes)
        before = self._trainable if self.training_initiated else None
        previous, self._trainable_asked = self._trainable_asked, (True, trainable)
        try:
            return method(self, *args, **keywords)
        finally:
            self._trainable_asked = previous
            if self.training_initiated and not self._ema_inside:
                self.set_trainable(before)
    return wrapper


def takes_param_groups(method):
    """Gives train() the keyword `param_groups` (NextFramePredictorS2S.set_param_groups: None or a sequence of (pattern,
    options) pairs).  train()'s parameter list is read by signature tests and stays as it is (takes_ema, takes_horizon,
    takes_trainable); the keyword is taken here, checked and resolved against the model's names on the host, before anything
    else runs, and held in self._groups_asked while the call runs.  train() applies it once the optimiser exists -- after
    initiate_training, which returns to no setting, when it has to make the optimiser itself -- and the setting that was in
    force before is back when the call ends, also after an exception.  Left out, the predictor's setting stays."""
    import functools
    from qtmpnn.groups import as_pairs

    @functools.wraps(method)
    def wrapper(self, *args, param_groups=_NOT_GIVEN, **keywords):
        if param_groups is _NOT_GIVEN:
            return method(self, *args, **keywords)
        self._check_param_groups(param_groups)  # (every refusal of set_param_groups but the one about the optimiser, which train() makes)
        before = self._groups if self.training_initiated else None
        previous, self._groups_asked = self._groups_asked, (True, param_groups)
        try:
            return method(self, *args, **keywords)
        finally:
            self._groups_asked = previous
            if self.training_initiated and not self._ema_inside:
                self.set_param_groups(as_pairs(before))
    return wrapper


class NextFramePredictor(ABC):
    """The abstract trainer facade of the reference (model/mpnnlstm.py:34-79; moving_mnist_example.ipynb cell 2 imports it):
    it holds the decomposition settings and names the three methods a predictor offers.  `thresh` is kept as given here;
    the concrete class turns `decompose=False` into thresh = -inf (:113)."""

    def __init__(self, thresh, experiment_name='experiment', decompose=True, input_features=1, transform_func=None,
                 condition='max_larger_than', device=None):
        self.experiment_name, self.device, self.model = experiment_name, device, None
        self.thresh, self.decompose = thresh, decompose
        self.transform_func, self.condition, self.input_features = transform_func, condition, input_features

    @abstractmethod
    def train(self, loader_train, loader_test, n_epochs=200, lr=0.01, lr_decay=0.95, mask=None):
        ...

    @abstractmethod
    def predict(self, x, mask=None, rollout=None):
        ...

    @abstractmethod
    def score(self, x, y, rollout=None):
        ...


class NextFramePredictorS2S(NextFramePredictor):
    def __init__(self, thresh, experiment_name='experiment', decompose=True, input_features=1, input_timesteps=3,
                 output_timesteps=3, device=None, transform_func=None, condition='max_larger_than', remesh_input=False,
                 binary=False, debug=False, model_kwargs={}):
        super().__init__(thresh=thresh, experiment_name=experiment_name, decompose=decompose, input_features=input_features,
                         transform_func=transform_func, condition=condition, device=device)
        # (output_timesteps itself is the horizon in force, a property: set_horizon; this keeps what the predictor was built with)
        self.input_timesteps, self.built_output_timesteps = input_timesteps, output_timesteps
        self.binary, self.debug = binary, debug
        self.thresh = thresh if decompose else -np.inf
        # As in the reference (:123-133) the Seq2Seq gets the RAW `thresh` (decompose=False changes self.thresh only) and
        # its transform_func / condition from model_kwargs alone (ice_exp.py:153-176 passes transform_func twice for that).
        self.model = Seq2Seq(input_features=input_features + 3,      # + positional encoding (x, y) + node size
                             input_timesteps=input_timesteps, output_timesteps=output_timesteps, thresh=thresh,
                             device=device, remesh_input=remesh_input, binary=binary, debug=debug,
                             **model_kwargs).to(device)
        self.training_initiated = False
        self.process_group = None
        self._output_days = {}          # (launch date, steps) -> the output days' indices into the normals (get_climatology_array)
        self._horizon_asked = None      # train()'s `horizon` while it runs (takes_horizon)
        self._launch_days = {}          # launch date -> its launch-state day's index (get_launch_climatology)
        self._asked = (None, None)      # the `references` / `launch_climatology` of the call that runs (takes_references)
        # what train()'s validation keywords leave (patience, restore_best, keep_best, monitor): see train()
        self.best_epoch = self.best_value = self.stopped_epoch = None
        self.monitor_history = []
        # the averaged weights (set_ema; None: off), the stash averaged_weights() keeps the live ones in, whether a block of it
        # is open, and train()'s (ema, ema_eval) while it runs (takes_ema)
        self.ema = self._ema_stash = None
        self._ema_inside, self._ema_asked = False, (None, True)
        # the selection of trainable parameters (set_trainable; None: all), its 0/1 mask over the flat vector (flat-vector
        # models with a selection; else None) and train()'s `trainable` while it runs (takes_trainable)
        self._trainable = self._train_mask = None
        self._trainable_asked = (False, None)
        # the parameter groups (set_param_groups; None: no setting) in check_groups' form, their vectors and launches
        # (qtmpnn.groups.GroupedStep, made on first use and kept with the optimiser) and train()'s `param_groups` while it runs
        self._groups = self._grouped = None
        self._groups_asked = (False, None)

    # -- trainable parameters (beyond the reference): qtmpnn.trainable has the pure parts ----------------------------------------
    def _check_trainable(self, patterns):
        """(patterns as a tuple or None, one flag per parameter name, whether the encoder cut applies), or the refusal: what
        qtmpnn.trainable.resolve_trainable refuses, an open averaged_weights() block, and the cut on a remesh_input=True model.
        Reads the predictor, changes nothing."""
        from qtmpnn.trainable import check_patterns, encoder_frozen, resolve_trainable
        names = [name for name, _, _ in name_table(self.model)]
        flags = resolve_trainable(names, patterns)
        if self._ema_inside:
            raise RuntimeError('trainable: set_trainable() inside averaged_weights(): leave the block first')
        cut = encoder_frozen(names, flags)
        if cut and self.model.remesh_input:
            raise NotImplementedError('trainable: a frozen encoder runs without autograd (the encoder cut), which does not cover '
                                      'remesh_input=True models (their encoder re-meshes between its steps); a selection that '
                                      'keeps one encoder parameter trainable only masks and is allowed')
        return check_patterns(patterns), names, flags, cut

    def set_trainable(self, patterns):
        """Train only the parameters some pattern of `patterns` matches; every other one is frozen.  patterns: None -- every
        parameter is trainable, the default, and every path is then what it was, bit for bit -- or a non-empty sequence of
        fnmatch patterns over the state-dict names (named_parameters(), qtmpnn.flat.name_table): ('decoder.*',),
        ('decoder.fc_out*', 'decoder.norm_o.*').  `trainable_names` lists what is trainable.

        A STEP UNDER A SELECTION is torch's own rule for requires_grad=False parameters: forward, loss and backward as ever; the
        frozen entries of the gradient are zero before the (all-reduced) gradient is used; the clipping norm is the norm of the
        trainable gradients; Adam updates the trainable entries; frozen parameters keep their bits.  Flat-vector models: one 0/1
        mask over the flat vector, made here, and ONE in-place multiplication of the gradient in _clip_and_step, the place every
        optimiser step goes through (train_step, accumulated_step, the truncated loop, both recompute modes, the captured steps --
        it sits in the graph that holds clip + Adam; under torch.distributed it follows the all-reduce, so no collective
        changes).  qt_flat_adam is untouched: with g = m = v = 0 its update is exactly 0.  Parameter-list models (torch's Adam):
        frozen parameters get requires_grad_(False) and grad = None, and the norm is taken over the trainable list.
        THE MOMENTS RULE: exp_avg and exp_avg_sq of every entry that is frozen are set to zero here, in place, before the next
        step -- Adam would otherwise go on moving a frozen entry along its old momentum.  An entry that is thawed later so
        restarts from zero moments under the shared step count (its bias corrections are those of the run's step, not of a new
        parameter's).
        THE ENCODER CUT: when no parameter under `encoder.` is trainable, the encoder phase of every rollout with autograd runs
        without it -- no activations kept, no backward launches for half of an I10O10 rollout's steps -- and loss, outputs,
        meshes, dropout masks and the decoder's gradients stay the plain step's, bit for bit (Seq2Seq.set_encoder_cut, which
        also says why there is no finer cut: a trainable head's gradient runs through every later decoder cell).  A partly
        frozen encoder keeps the whole graph; only the masking applies.
        The setting follows the optimiser, as the average does: initiate_training() returns to all-trainable.  It is no training
        state: checkpoints neither store nor restore it (frozen moments are zero in the file, so load_checkpoint followed by the
        same set_trainable continues bit for bit).  The average (set_ema) is untouched: the shadow of a frozen parameter is the
        same recurrence on a constant.  A CAPTURED STEP KEEPS THE SETTING IT WAS CAPTURED UNDER and refuses to run
        (RuntimeError, `trainable`) once the predictor's is another one.  predict, verify, the products and sensitivity do not
        look at the setting.
        Refusals, each under `trainable`, before any launch and before anything changes: TypeError for a plain string, for
        what is no sequence and for a pattern that is no string; ValueError for an empty sequence, a pattern that matches no
        name (it lists the top-level names), a selection that leaves nothing trainable, and a predictor without
        initiate_training() / train(); RuntimeError inside averaged_weights(); NotImplementedError where the cut would apply
        to a remesh_input=True model."""
        from qtmpnn.trainable import flat_mask
        patterns, names, flags, cut = self._check_trainable(patterns)
        if patterns is not None and not self.training_initiated:
            raise ValueError('trainable: the selection follows the optimiser: call initiate_training() first (or pass '
                             'train(trainable=patterns))')
        if not self.training_initiated:
            return                          # (None on a predictor without an optimiser: all-trainable is what it is)
        # (the same selection again keeps its mask: a captured step reads it through its pointer)
        keep = self._train_mask if patterns == self._trainable else None
        flat = self.flat is not None
        if flat and not self.flat.intact(self.model):
            raise RuntimeError('the model parameters were moved or replaced after initiate_training(): call it again')
        with torch.no_grad():
            if flat:
                mask = None if patterns is None else keep if keep is not None else flat_mask(name_table(self.model), flags,
                                                                                             self.flat.param.device)
                st = self.optimizer.state.get(self.flat.param)
                if st and mask is not None:
                    frozen = mask == 0
                    st['exp_avg'].masked_fill_(frozen, 0.0)
                    st['exp_avg_sq'].masked_fill_(frozen, 0.0)
                self._train_mask = mask
            else:
                self._share_step_count()
                for p, f in zip(self.model.parameters(), flags, strict=True):
                    p.requires_grad_(f)
                    if not f:
                        p.grad = None
                        st = self.optimizer.state.get(p)
                        if st:
                            st['exp_avg'].zero_()
                            st['exp_avg_sq'].zero_()
                self._train_mask = None
        self._trainable = patterns
        self.model.set_encoder_cut(cut)
        self._refresh_groups()              # (set_param_groups: a frozen entry gets neither decay nor blend)

    def _share_step_count(self):
        """Parameter-list models: torch's Adam counts steps per parameter and skips one without a gradient, so a frozen
        parameter's count stands still.  Its moments are zero, so the count means nothing until it is thawed; the largest count
        is written into every one that exists, in place: ONE step count, what a checkpoint stores and what a thawed entry
        continues under."""
        states = [st for st in (self.optimizer.state.get(p) for p in self.model.parameters()) if st]
        steps = [float(st['step']) for st in states]
        if steps and min(steps) != max(steps):
            for st in states:
                st['step'].fill_(max(steps))

    @property
    def trainable_names(self):
        """The names of the trainable parameters, a tuple in state-dict order (all of them without a selection)."""
        from qtmpnn.trainable import resolve_trainable
        names = [name for name, _, _ in name_table(self.model)]
        return tuple(n for n, f in zip(names, resolve_trainable(names, self._trainable)) if f)

    @contextlib.contextmanager
    def training_only(self, patterns):
        """`with nfp.training_only(('decoder.*',)):` -- set_trainable(patterns) for the block; the previous selection is back
        afterwards, also after an exception (the moments of what it freezes are zeroed then, by the same rule).  Blocks nest:
        the inner one holds while it runs."""
        previous = self._trainable
        self.set_trainable(patterns)
        try:
            yield self
        finally:
            self.set_trainable(previous)

    def _trainable_guard(self, held):
        """Before a replay of a step captured under the selection `held`: refused unless that still is the predictor's (the
        mask multiplication, the list of stepped parameters and the encoder cut are part of the capture)."""
        if held != self._trainable:
            raise RuntimeError(f'trainable: this step was captured under trainable={held!r} and the predictor is now at '
                               f'trainable={self._trainable!r}: a captured step keeps the setting it was captured under; capture '
                               'a new one')

    # -- parameter groups (beyond the reference): qtmpnn.groups has the pure parts and the launches ------------------------------
    def _check_param_groups(self, groups):
        """(the setting in check_groups' form or None, {name: (lr_scale, weight_decay)}), or the refusal: what
        qtmpnn.groups.resolve_groups refuses, and an open averaged_weights() block.  Reads the predictor, changes nothing."""
        from qtmpnn.groups import check_groups, resolve_groups
        resolved = resolve_groups([name for name, _, _ in name_table(self.model)], groups)
        if self._ema_inside:
            raise RuntimeError('param_groups: set_param_groups() inside averaged_weights(): leave the block first')
        return check_groups(groups), resolved

    def set_param_groups(self, groups):
        """A learning-rate scale and a decoupled weight decay per parameter.  groups: None -- no setting, the default, and every
        path is then what it was, bit for bit -- or a non-empty sequence of (pattern, options) pairs (a dict pattern -> options
        is read in its insertion order): `pattern` an fnmatch pattern over the state-dict names, the names set_trainable
        matches; `options` a dict with keys from {'lr_scale', 'weight_decay'}, finite numbers >= 0.  The FIRST matching pair
        decides a parameter; one that nothing matches has lr_scale 1 and weight_decay 0.  `param_group_table` lists the result.
            [('*norm*', {}), ('*bias*', {}), ('encoder.*', dict(lr_scale=0.1, weight_decay=1e-2)), ('*', dict(weight_decay=1e-2))]
        A STEP UNDER A SETTING is torch's AdamW with the learning rate lr * s_i and the decay lam_i per entry, lr the optimiser's
        current learning rate (the device tensor when capturable: StepLR is followed by replays); after the all-reduce, after
        the trainable mask and after clipping with the GLOBAL norm, which is unchanged:
            p_i <- p_i * (1 - lr * s_i * lam_i);    p_i <- p_i - lr * s_i * mhat_i / (sqrt(vhat_i) + eps)
        with the moments and the one step count updated exactly as without a setting, for every entry, also where s_i = 0.
        qtmpnn.groups.GroupedStep has the mechanism, ONE for both optimiser forms, in _clip_and_step, the place every optimiser
        step goes through: multiply by the decay vector, stash the parameters in a buffer allocated once, run the existing step
        untouched (qt_flat_adam, torch's fused Adam; optimizer.param_groups stays ONE group), blend p <- p0 + s (p - p0) on the
        entries with s != 1.  No host read, no allocation per step; the launches sit in the graph that holds clip + Adam.
        WHAT HOLDS: entries with (s, lam) = (1, 0) have the plain step's bits in one step from equal state (the decay
        multiplies by exactly 1.0f and the blend skips them); a setting that is (1, 0) everywhere issues no launch at all;
        entries with s = 0 keep their bits while their moments advance and the clipping norm still sees them (this is not
        set_trainable); entries frozen by set_trainable get neither decay nor update; the average (set_ema) is updated after
        the blend, so the shadow averages what the step wrote.
        The setting follows the optimiser: initiate_training() returns to None.  It is no training state: checkpoints neither
        store nor restore it.  A CAPTURED STEP KEEPS THE SETTING IT WAS CAPTURED UNDER and refuses to run (RuntimeError,
        `param_groups`) once the predictor's is another one.  predict, verify, the products and sensitivity do not look at it.
        Refusals, each under `param_groups`, before any launch and before anything changes: TypeError for a plain string, for
        what is no sequence, for a pair that is no (str, dict) and for an option that is no number (True included); ValueError
        for an empty sequence, an unknown option key, a negative or non-finite number, a pattern that is the first match of no
        parameter (it lists the top-level names and says when an earlier pattern shadows it), and a predictor without
        initiate_training() / train(); RuntimeError inside averaged_weights()."""
        from qtmpnn.groups import GroupedStep
        setting, _ = self._check_param_groups(groups)
        if setting is not None and not self.training_initiated:
            raise ValueError('param_groups: the setting follows the optimiser: call initiate_training() first (or pass '
                             'train(param_groups=groups))')
        if not self.training_initiated:
            return                          # (None on a predictor without an optimiser: no setting is what it has)
        if setting is not None and self._grouped is None:
            if self.flat is not None and not self.flat.intact(self.model):
                raise RuntimeError('the model parameters were moved or replaced after initiate_training(): call it again')
            # (made once per optimiser and filled in place from then on: a captured step reads the vectors by pointer)
            self._grouped = GroupedStep(self.flat.param if self.flat is not None else list(self.model.parameters()),
                                        name_table(self.model))
        self._groups = setting
        self._refresh_groups()

    def _refresh_groups(self):
        """Fill the vectors of the setting in force under the trainable selection in force (set_param_groups and set_trainable
        end here: a frozen entry gets neither decay nor blend)."""
        if self._groups is None or self._grouped is None:
            return
        from qtmpnn.groups import as_pairs, resolve_groups
        from qtmpnn.trainable import resolve_trainable
        names = [name for name, _, _ in name_table(self.model)]
        self._grouped.set(resolve_groups(names, as_pairs(self._groups)), resolve_trainable(names, self._trainable))

    @property
    def param_group_table(self):
        """{state-dict name: (lr_scale, weight_decay)} of the setting in force, in state-dict order ((1.0, 0.0) without one)."""
        from qtmpnn.groups import as_pairs, resolve_groups
        return resolve_groups([name for name, _, _ in name_table(self.model)], as_pairs(self._groups))

    def _groups_guard(self, held):
        """Before a replay of a step captured under the setting `held`: refused unless that still is the predictor's (the
        decay, stash and blend launches are part of the capture)."""
        if held != self._groups:
            from qtmpnn.groups import as_pairs
            raise RuntimeError(f'param_groups: this step was captured under param_groups={as_pairs(held)!r} and the predictor is '
                               f'now at param_groups={as_pairs(self._groups)!r}: a captured step keeps the setting it was '
                               'captured under; capture a new one')

    # -- averaged weights (beyond the reference): qtmpnn.ema.WeightEMA, updated after every optimiser step ----------------------
    def set_ema(self, decay):
        """Keep an exponential moving average of the weights: after EVERY optimiser step s <- decay * s + (1 - decay) * p
        (qtmpnn.ema.WeightEMA has the op sequence; _clip_and_step is the one place every step goes through: train_step,
        accumulated_step -- one update per optimiser step, none per micro-batch --, every chunk of the truncated loop, the
        captured steps, both recompute modes; under torch.distributed the update follows the all-reduce, so every rank keeps
        the same shadow without a collective).  decay: a float in [0, 1); None (the default state) switches the average off
        and drops its state, and every path is then what it was, bit for bit.  The same decay again keeps the state, another one
        starts anew; initiate_training() drops it with the optimiser.  Training itself never reads the average:
        averaged_weights(), apply_ema() and train(ema=, ema_eval=) do, and save_checkpoint() stores it.
        A CAPTURED STEP KEEPS THE SETTING IT WAS CAPTURED UNDER, as it keeps its recompute mode -- the update is part of the
        graph that holds clip + Adam -- and refuses to run (RuntimeError, `ema`) once the predictor's setting is another one.
        Refusals, before any launch: TypeError for what is no number (True included), ValueError for a decay outside [0, 1)
        or a NaN, and for a predictor without initiate_training() / train()."""
        from qtmpnn.ema import WeightEMA, check_decay
        if decay is not None:
            decay = check_decay(decay)
            if not self.training_initiated:
                raise ValueError('ema: the average follows the optimiser: call initiate_training() first (or pass train(ema=decay))')
        if self._ema_inside:
            raise RuntimeError('ema: set_ema() inside averaged_weights(): leave the block first')
        if decay is None:
            self.ema = self._ema_stash = None
        elif self.ema is None or self.ema.decay != decay:
            self.ema = WeightEMA(self.flat.param if self.flat is not None else list(self.model.parameters()), decay)

    def _live_weights(self):
        """The parameters as the average sees them, detached: the flat tensor, or the list."""
        if self.flat is not None:
            if not self.flat.intact(self.model):
                raise RuntimeError('the model parameters were moved or replaced after initiate_training(): call it again')
            return self.flat.param.detach()
        return [p.detach() for p in self.model.parameters()]

    @contextlib.contextmanager
    def averaged_weights(self):
        """`with nfp.averaged_weights():` -- the model runs on the averaged weights inside the block.  On entry the live
        parameters are copied to a stash (allocated on first use, kept) and WeightEMA.averaged() is written into the parameters
        IN PLACE: the flat buffer keeps its views and its zero pad tail, and every capture that reads the parameters by pointer
        (predict(use_graph=True), verify, train()'s test_graph captures, a make_graphed_rollout made before) works unchanged
        inside.  On exit, also after an exception, the live parameters are copied back: bit for bit what they were.  Refused by
        name (`ema`): no average (set_ema), no optimiser step averaged yet, a nested block; and inside the block every
        optimiser step, set_ema and apply_ema."""
        if self.ema is None:
            raise ValueError('ema: averaged_weights() needs averaged weights: call set_ema(decay) (or train(ema=decay)) first')
        if self._ema_inside:
            raise RuntimeError('ema: averaged_weights() is not re-entrant: the block is already open')
        self.ema.divisor()              # (refuses an average of no step before anything is copied)
        live = self._live_weights()         # (detached: the copies below are no autograd operations)
        if self._ema_stash is None:
            self._ema_stash = torch.empty_like(live) if torch.is_tensor(live) else [torch.empty_like(p) for p in live]
        copy = (lambda dst, src: dst.copy_(src)) if torch.is_tensor(live) else torch._foreach_copy_
        copy(self._ema_stash, live)
        self._ema_inside = True
        try:
            self.ema.averaged(live)
            yield self
        finally:
            copy(live, self._ema_stash)
            self._ema_inside = False

    def apply_ema(self):
        """Copy the averaged weights into the parameters for good (in place), for save() and export: the live weights are gone
        then, the average and the optimiser are left as they are.  save() / load() themselves are what they were."""
        if self.ema is None:
            raise ValueError('ema: apply_ema() needs averaged weights: call set_ema(decay) (or train(ema=decay)) first')
        if self._ema_inside:
            raise RuntimeError('ema: apply_ema() inside averaged_weights(): leave the block first')
        self.ema.averaged(self._live_weights())

    def _ema_guard(self, captured=False, ema=None):
        """Before an optimiser step: refused inside averaged_weights() (the step would move the averaged weights and the exit
        would throw it away); captured: the step is a replay of a capture that was made while the average was `ema` (None:
        off) -- refused unless that still is the predictor's."""
        if self._ema_inside:
            raise RuntimeError('ema: an optimiser step inside averaged_weights(): the parameters are the averaged ones there')
        if captured and ema is not self.ema:
            say = lambda e: 'ema=None' if e is None else f'ema={e.decay!r}'
            raise RuntimeError(f'ema: this step was captured under {say(ema)} and the predictor is now at {say(self.ema)}'
                               + (' (set anew)' if ema is not None and self.ema is not None and ema.decay == self.ema.decay else '')
                               + ': a captured step keeps the setting it was captured under; capture a new one')

    # -- activation recomputation (beyond the reference): the mode lives on the Seq2Seq, where the rollout is -------------------
    @property
    def recompute(self):
        return self.model.recompute

    def set_recompute(self, mode):
        """How the rollouts that build an autograd graph keep their activations: None (default) -- every step's until the
        backward -- 'step' or 'stream' -- only what crosses a step boundary; every encoder and decoder step is then re-run, one at
        a time, while the backward passes it (Seq2Seq.set_recompute has the details).  forward_loss, train_step,
        accumulated_step / accumulate_gradients, every chunk of truncated_backward, make_graphed_step and train honour it; loss,
        gradients and parameters are the plain step's bit for bit, for one more forward's launches.  What autograd keeps from
        the forward shrinks to the boundaries; the peak shrinks less, because the deferred weight gradient still holds every
        step's Chebyshev planes and gate gradients from that step's backward to the pass's last one (README has the measured
        figures).  'stream' is 'step' without that hold: every use's weight gradient is reduced inside its own backward and added
        to a running sum, so the peak no longer grows with those operands; the weight gradients are then the plain step's up to
        rounding (another order of additions, fixed: two runs give the same bits), everything else stays bit for bit, and the step
        takes one short launch per step and weight instead of one grouped launch.  A CAPTURED STEP KEEPS THE MODE IT WAS
        CAPTURED UNDER: changing the mode afterwards affects new captures only.  Passes without autograd (predict, verify and its products, attention_weights, the test pass
        of train) do not look at it.  The mode is no training state: checkpoints neither store nor restore it.  Any other value:
        ValueError, before anything is launched."""
        self.model.set_recompute(mode)

    @contextlib.contextmanager
    def recomputing(self, mode):
        """`with nfp.recomputing('step'):` (or 'stream', None) -- set_recompute(mode) for the block; the previous mode is back
        afterwards, also after an exception."""
        previous = self.recompute
        self.set_recompute(mode)
        try:
            yield self
        finally:
            self.model.set_recompute(previous)

    # -- rollout horizon (beyond the reference): the setting lives on the Seq2Seq, where the rollout is ---------------------------
    @property
    def output_timesteps(self):
        """The output steps every method rolls out: the horizon in force (set_horizon), else built_output_timesteps."""
        return self.model.horizon

    def set_horizon(self, k):
        """Roll out k output steps from now on; None: the steps the predictor was built with (built_output_timesteps) again.
        The weights do not depend on the step count, so while a horizon k is in force EVERY METHOD IS THE SAME METHOD OF A
        PREDICTOR BUILT WITH output_timesteps=k THAT HOLDS THE SAME PARAMETERS, bit for bit: forward_loss, train_step,
        accumulated_step, truncated_backward, make_graphed_step (accumulate=k too) and both recompute modes; predict, verify,
        every product and its make_graphed_* maker, sensitivity and attention_weights.  `output_timesteps` reads k then.
        k at or below the steps y holds: the first k steps of y are read in place, as a view (qtmpnn.horizon.first_steps; the
        kernels take the clip stride).  k above the built value is allowed: the loader or the caller then supplies y with at
        least k steps (a ClipBank made with output_timesteps=k); what reads no y (predict) needs none.  get_climatology_array
        gives k days; lead_weights must have length k; event_dates(persist=), sensitivity(leads=) and the references are held to
        k.  A y or a hand-made concat_layers with fewer than k steps is refused (ValueError, `horizon`) before any launch.
        A CAPTURED STEP OR PRODUCT KEEPS THE HORIZON IT WAS CAPTURED UNDER, as it keeps its recompute mode; its replay takes y
        with at least that many steps.  The horizon is no training state: checkpoints neither store nor restore it, and their
        description keeps the built value.  It changes no weights, so it may be set inside averaged_weights().  Anything but
        None or an integer >= 1 is refused by name (qtmpnn.horizon.check_horizon) before anything is launched."""
        self.model.set_horizon(k)

    @contextlib.contextmanager
    def horizon(self, k):
        """`with nfp.horizon(k):` -- set_horizon(k) for the block; the previous setting is back afterwards, also after an
        exception.  Blocks nest: the inner one holds while it runs."""
        previous = self.model.__dict__.get('_horizon')
        self.set_horizon(k)
        try:
            yield self
        finally:
            self.model.set_horizon(previous)

    def _first_steps(self, y, concat_layers=None, held=None):
        """(y, concat_layers) held to the step count in force: the first k steps of each, as views.  While a horizon is set, fewer
        than k steps are refused under `horizon`; with none set a short tensor goes on as it is, to the shape checks that were
        there before.  held: the (k, whether a horizon was set) a capture was made under, `self._held()` then, in place of the
        setting in force.  Host code: it comes before the launches of whatever calls it."""
        k, strict = self._held() if held is None else held
        return first_steps(y, k, 'y', strict), first_steps(concat_layers, k, 'concat_layers', strict)

    def _held(self):
        """(the step count in force, whether a horizon is set): what a capture keeps for its replays (_first_steps)."""
        return self.output_timesteps, self.model.__dict__.get('_horizon') is not None

    # -- small helpers of the reference ---------------------------------------------
    def get_n_params(self):
        return get_n_params(self.model)

    def save(self, directory):
        torch.save(self.model.state_dict(), os.path.join(directory, f'{self.experiment_name}.pth'))

    def load(self, directory):
        path = os.path.join(directory, f'{self.experiment_name}.pth')
        self.model.load_state_dict(torch.load(path, map_location=self.device or 'cpu', weights_only=True))

    # -- checkpoints: everything a resumed run needs to continue bit for bit (beyond the reference) ------------------------------
    def _description(self):
        """What a checkpoint must agree with before it is loaded: the settings that fix the parameter set, and the set itself."""
        m = self.model
        return {'convolution_type': m.convolution_type, 'hidden_size': int(m.hidden_size), 'n_layers': int(m.n_layers),
                'n_conv_layers': int(m.encoder.rnns[0].n_conv_layers), 'input_features': int(self.input_features),
                'input_timesteps': int(self.input_timesteps), 'output_timesteps': int(self.built_output_timesteps),
                'binary': bool(self.binary), 'parameters': [[name, list(shape)] for name, _, shape in name_table(m)]}

    def save_checkpoint(self, path):
        """Write the whole training state to the file `path` (torch.save of a dict of host tensors and plain Python values: it
        loads with torch.load(path, weights_only=True)), so that load_checkpoint + train(n_epochs=k) continues this run bit for bit:

            format        1; 2 when averaged weights are kept (set_ema), and only then
            description   convolution_type, hidden_size, n_layers, n_conv_layers, input_features, input_timesteps,
                          output_timesteps, binary, parameters [[name, shape], ...] in module order
            state_dict    model.state_dict(), the keys and values save() writes
            optimizer     exp_avg / exp_avg_sq {name: tensor in the parameter's shape}, step (one integer), lr (float), betas, eps:
                          one layout for FlatAdam and torch's Adam (qtmpnn.optim.adam_state), so either loads the other's file
            scheduler     StepLR.state_dict(), learning rates as floats
            train_loss, test_loss, capturable
            rng           torch (torch.get_rng_state()), cuda (torch.cuda.get_rng_state(device), None on the CPU), attention
                          (ops.dropout_state: the call counter and device step counter the attention kernels' seeds are made of)
            ema           format 2 only: shadow {name: tensor in the parameter's shape}, decay, updates (WeightEMA.state: one
                          layout for the flat shadow and the per-parameter one, so either loads the other's file)

        The file is written under a temporary name beside `path` and moved there by os.replace: an interrupted save leaves
        whatever was under `path` as it was.  Under torch.distributed the ranks hold the same state: one rank saves."""
        if not self.training_initiated:
            raise ValueError('save_checkpoint: nothing to resume yet (no initiate_training() / train()); save() stores the weights')
        from qtmpnn.optim import adam_state
        if self.flat is None and self._trainable is not None:
            self._share_step_count()        # (frozen parameters' counts stand still under torch's Adam; the file holds one)
        group = self.optimizer.param_groups[0]
        dev = next(self.model.parameters()).device
        host = lambda v: float(v) if torch.is_tensor(v) else [host(e) for e in v] if isinstance(v, (list, tuple)) else v
        if self._ema_inside:
            raise RuntimeError('ema: save_checkpoint() inside averaged_weights(): the parameters are the averaged ones there')
        ckpt = {'format': 1 if self.ema is None else 2, 'description': self._description(),
                'state_dict': {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
                'optimizer': adam_state(self.optimizer, self.model),
                'scheduler': {k: host(v) for k, v in self.scheduler.state_dict().items()},
                'train_loss': [float(v) for v in self.train_loss], 'test_loss': [float(v) for v in self.test_loss],
                'capturable': bool(group.get('capturable', False)),
                'rng': {'torch': torch.get_rng_state(), 'cuda': torch.cuda.get_rng_state(dev) if dev.type == 'cuda' else None,
                        'attention': ops.dropout_state(dev)}}
        if self.ema is not None:
            ckpt['ema'] = self.ema.state(self.model)
        path = os.fspath(path)
        tmp = f'{path}.tmp{os.getpid()}'
        try:
            torch.save(ckpt, tmp)
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise

    def _checked_checkpoint(self, path):
        """The checkpoint under `path`, host tensors, or a ValueError that names the field that does not fit this predictor.
        Reads the file and this predictor, changes neither."""
        from qtmpnn.ema import check_state
        from qtmpnn.optim import check_adam_state
        ckpt = torch.load(path, map_location='cpu', weights_only=True)
        if not isinstance(ckpt, dict) or 'format' not in ckpt:
            raise ValueError(f"format: {path} is no checkpoint of save_checkpoint() (no 'format' entry; load() reads the weights of save())")
        if not isinstance(ckpt['format'], int) or ckpt['format'] > CHECKPOINT_FORMAT or ckpt['format'] < 1:
            raise ValueError(f"format: the file has format {ckpt['format']!r}, this version reads up to {CHECKPOINT_FORMAT}")
        for k in ('description', 'state_dict', 'optimizer', 'scheduler', 'train_loss', 'test_loss', 'capturable', 'rng'):
            if k not in ckpt:
                raise ValueError(f'{k}: missing in the file')
        if ckpt['format'] >= 2 and 'ema' not in ckpt:
            raise ValueError(f"format: the file has format {ckpt['format']} and no 'ema': format 2 is format 1 with averaged weights")
        if ckpt['format'] < 2 and 'ema' in ckpt:
            raise ValueError(f"ema: averaged weights in a file of format {ckpt['format']}: they belong to format 2")
        here, there = self._description(), ckpt['description']
        for k, v in here.items():
            if k != 'parameters' and there.get(k) != v:
                raise ValueError(f'{k}={there.get(k)!r} in the file, {v!r} here')
        mine, theirs = {n: tuple(s) for n, s in here['parameters']}, {n: tuple(s) for n, s in there.get('parameters', [])}
        missing, extra = [n for n in mine if n not in theirs], [n for n in theirs if n not in mine]
        if missing or extra or list(mine) != list(theirs):
            raise ValueError(f'parameters: the names differ: missing in the file {missing}, not in this model {extra}'
                             + ('' if missing or extra else ' (same names, another order)'))
        for n, s in mine.items():
            if theirs[n] != s:
                raise ValueError(f'parameters[{n!r}]: shape {theirs[n]} in the file, {s} here')
        sd, own = ckpt['state_dict'], self.model.state_dict()
        missing, extra = [k for k in own if k not in sd], [k for k in sd if k not in own]
        if missing or extra:
            raise ValueError(f'state_dict: the keys differ: missing in the file {missing}, not in this model {extra}')
        for k, v in own.items():
            if not torch.is_tensor(sd[k]) or tuple(sd[k].shape) != tuple(v.shape):
                raise ValueError(f'state_dict[{k!r}]: shape {tuple(sd[k].shape) if torch.is_tensor(sd[k]) else None} in the file, '
                                 f'{tuple(v.shape)} here')
        check_adam_state(ckpt['optimizer'], name_table(self.model))
        if 'ema' in ckpt:
            check_state(ckpt['ema'], name_table(self.model))
        sched = ckpt['scheduler']
        for k in ('last_epoch', '_last_lr', 'step_size', 'gamma', 'base_lrs'):
            if not isinstance(sched, dict) or k not in sched:
                raise ValueError(f'scheduler: no {k!r}')
        if len(ckpt['train_loss']) != len(ckpt['test_loss']):
            raise ValueError(f"train_loss: {len(ckpt['train_loss'])} epochs, test_loss has {len(ckpt['test_loss'])}")
        rng = ckpt['rng']
        for k in ('torch', 'cuda', 'attention'):
            if not isinstance(rng, dict) or k not in rng:
                raise ValueError(f'rng: no {k!r}')
        return ckpt

    @on_device(lambda self, *a, **k: self.device)
    def load_checkpoint(self, path, capturable=None):
        """Restore what save_checkpoint(path) wrote into this predictor; `train(n_epochs=k)` then continues that run: the same
        parameters and losses, bit for bit, as the run that was never interrupted, and `self.loss` covers the restored epochs and
        the new ones.

        A predictor that has not trained yet gets initiate_training() first.  capturable: None takes the mode the file was
        written in; True / False converts (the learning rate becomes a device tensor or a float, the step counter moves with
        it), so an eager run resumes with train(use_graph=True) and the other way round.  A predictor whose optimiser is in
        the other mode than the one asked for is initiated again; its captured steps, if any, are void then.

        Otherwise EVERYTHING IS RESTORED IN PLACE: parameters (load_state_dict copies into them; the flat buffer keeps its views
        and its zero pad tail), Adam moments, step counters, a device learning rate and the attention-dropout counter by copy_ /
        fill_ into the storage that is there.  A make_graphed_step object captured before the load holds pointers into
        exactly these buffers: it keeps working and its next replay continues from the loaded state.  The weight packing reads
        the parameters in every forward pass, so nothing else has to be told.  Averaged weights (set_ema) follow the file: with an
        average of the file's decay active the shadow is loaded in place and the count taken; otherwise the average is made with the
        file's decay; a file without one switches it off.

        A file that does not fit is refused with a ValueError that names the field -- no checkpoint, a newer format, another
        description (`convolution_type='ChebConv' in the file, 'GCNConv' here`), parameter names, shapes, non-finite moments,
        negative exp_avg_sq, step < 0, averaged weights that do not fit -- after reading the file on the host and before anything here changes.  Every rank of a
        torch.distributed run loads the same file; there is no collective."""
        from qtmpnn.optim import load_adam_state, set_lr
        if self._ema_inside:
            raise RuntimeError('ema: load_checkpoint() inside averaged_weights(): leave the block first')
        ckpt = self._checked_checkpoint(path)
        opt, sched = ckpt['optimizer'], dict(ckpt['scheduler'])
        want = bool(ckpt['capturable']) if capturable is None else bool(capturable)
        if not self.training_initiated or bool(self.optimizer.param_groups[0].get('capturable', False)) != want:
            self.initiate_training(opt['lr'], sched['gamma'], capturable=want)
        self.model.load_state_dict(ckpt['state_dict'])          # (copy_ into the parameters, as load() does)
        if self.flat is not None and not self.flat.intact(self.model):
            raise RuntimeError('the model parameters were moved or replaced after initiate_training(): call it again')
        load_adam_state(self.optimizer, self.model, opt)
        self.set_ema(ckpt['ema']['decay'] if 'ema' in ckpt else None)       # (an average of that decay stays where it is)
        if self.ema is not None:
            self.ema.load_state(ckpt['ema'])
        group = self.optimizer.param_groups[0]
        set_lr(group, 'initial_lr', sched['base_lrs'][0])
        sched['base_lrs'], sched['_last_lr'] = [group['initial_lr']], [group['lr']]     # (the scheduler's own aliases)
        self.scheduler.load_state_dict(sched)
        self.train_loss, self.test_loss = list(ckpt['train_loss']), list(ckpt['test_loss'])
        self.monitor_history = []           # (no checkpoint field: a Monitor's patience count starts anew after a load)
        rng, dev = ckpt['rng'], next(self.model.parameters()).device
        torch.set_rng_state(rng['torch'])
        if dev.type == 'cuda' and rng['cuda'] is not None:
            torch.cuda.set_rng_state(rng['cuda'], dev)
        ops.set_dropout_state(rng['attention'], dev)

    def test_threshold(self, x, thresh, mask=None, high_interest_region=None, contours=True):
        import matplotlib.pyplot as plt
        n_sample, w, h, _ = x.shape
        graph = image_to_graph(add_positional_encoding(x), thresh=thresh, mask=mask, high_interest_region=high_interest_region,
                               transform_func=self.transform_func)
        mesh = graph['mapping']
        rec = unflatten(graph['data'][..., [0]], mesh, (w, h)).cpu()
        fig, axs = plt.subplots(1, n_sample, figsize=(5 * n_sample, 4), squeeze=False)
        for i in range(n_sample):
            axs[0, i].imshow(rec[i, ..., 0])
            if contours:
                plot_contours(axs[0, i], mesh.labels[0].cpu().numpy())
        plt.suptitle(f'Threshold: {thresh} | Num. nodes: {mesh.N}')
        return fig, axs[0]

    @on_device(lambda self, *a, **k: self.device)
    def initiate_training(self, lr, lr_decay, capturable=False):
        self.loss_func_name = 'MSE' if not self.binary else 'BCE'
        # (the selection of trainable parameters follows the optimiser: a new one starts with all of them)
        for p in self.model.parameters():
            p.requires_grad_(True)
        self._trainable = self._train_mask = None
        self.model.set_encoder_cut(False)
        self._groups = self._grouped = None     # (and so do the parameter groups: set_param_groups)
        if capturable:      # optimizer.step() inside a hipGraph needs device-side step counters and lr
            lr = torch.tensor(float(lr), device=self.device)
        # fused: one multi-tensor kernel for all 238 parameter tensors (the default per-tensor path costs ~1000 tiny
        # launches per step once the step counters live on the device)
        fused = self.device is not None and torch.device(self.device).type == 'cuda'
        # Plain ChebConv models on the GPU: every parameter is a view of one flat buffer and the backward pass returns one
        # flat gradient vector (qtmpnn.flat), so the optimizer sees ONE tensor -- Adam is elementwise, and the clipping norm is
        # the norm of all gradients either way, so the update is the reference's; only the launch count differs (two launches
        # for clip + Adam instead of ~25, the all-reduce without a gather copy).
        self.flat = None
        if fused and self.model.encoder.plannable and self.model.decoder.plannable:
            self.flat = flat_params(self.model)
        if self.flat is not None:
            from qtmpnn.optim import FlatAdam
            self.optimizer = FlatAdam(self.flat.param, lr=lr, capturable=capturable)      # clip + Adam in two launches
        else:
            self.optimizer = torch.optim.Adam(self.model.parameters(), lr=lr, capturable=capturable, fused=fused or None)
        self.scheduler = StepLR(self.optimizer, step_size=3, gamma=lr_decay)
        self.writer = SummaryWriter('runs/' + self.experiment_name + '_' + datetime.datetime.now().strftime('%Y%m%d_%H_%M_%S'))
        self.test_loss, self.train_loss = [], []
        self.monitor_history = []
        self.ema = self._ema_stash = None       # (the average follows the optimiser: set_ema() starts a new one)
        self.training_initiated = True

    # -- the measured unit -----------------------------------------------------------
    def forward_loss(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                     fused=False, pos_weight=None, loss_weights=None, lead_weights=None):
        """loss_weights (W, H) / lead_weights (T_out,): the weighted loss of masked_mse (checked before the rollout starts).
        fused=True (binary predictors only): the fused binary cross-entropy of masked_mse.  On a binary=True predictor any of
        loss_weights / lead_weights / pos_weight (the positive-class weight) selects masked_bce, which is always fused."""
        self._check_fused(fused)
        check_concat_clips(x, concat_layers)
        y, concat_layers = self._first_steps(y, concat_layers)
        lw = self._loss_weights(x, mask, loss_weights, lead_weights, pos_weight)
        y_hat, meshes = self.model(x, y, concat_layers, teacher_forcing_ratio=0, mask=mask,
                                   high_interest_region=high_interest_region, graph_structure=graph_structure)
        if lw is None:
            return masked_mse(y_hat, meshes, y, mask, self.binary, fused=fused)
        return self._weighted_loss(y_hat, meshes, y, mask, lw)

    def _check_fused(self, fused):
        if fused and not self.binary:
            raise ValueError('fused: fused=True selects the fused binary cross-entropy and needs a binary=True predictor')

    def _loss_weights(self, x, mask, loss_weights, lead_weights, pos_weight=None, shape=None, steps=None):
        """The checked, uploaded weights of this predictor's loss for batches shaped like x, or of frames of `shape` (None:
        unweighted).  A binary=True predictor takes pos_weight beside them (masked_bce); any other refuses it by name.
        steps: the length lead_weights must have (None: the horizon in force; train(horizon=) gives the built step count and
        cuts the weights to every epoch's horizon, _horizon_weights)."""
        shape = tuple(x.shape[-3:-1]) if shape is None else tuple(shape)
        if (steps is not None or self._held()[1]) and (isinstance(lead_weights, (list, tuple))
                                                       or getattr(lead_weights, 'ndim', None) == 1):
            want = self.output_timesteps if steps is None else steps
            if len(lead_weights) != want:       # (said under `horizon` while one is at work; LossWeights checks everything else)
                raise ValueError(f'horizon: lead_weights has {len(lead_weights)} entries, ' + (
                    f'horizon={want} needs {want}' if steps is None else
                    f'train(horizon=) takes the built length {want} and cuts it to the first entries of every epoch\'s horizon'))
        steps = self.output_timesteps if steps is None else steps
        if self.binary:
            lw = bce_weights_of(loss_weights, lead_weights, pos_weight, shape, steps, mask)
        elif pos_weight is not None:
            raise ValueError('pos_weight: the positive-class weight belongs to the binary cross-entropy and needs a binary=True predictor')
        else:
            lw = loss_weights_of(loss_weights, lead_weights, shape, steps, mask)
        return lw if lw is None else lw.to(self.device if self.device is not None else ('cpu' if x is None else x.device))

    def _weighted_loss(self, y_hat, meshes, y, mask, lw):
        """The weighted loss of this predictor's head (weighted_loss)."""
        return weighted_loss(y_hat, meshes, y, mask, lw, self.binary)

    def zero_grad(self):
        """Drop all gradients (set to None, like optimizer.zero_grad(set_to_none=True) on the reference's per-tensor optimizer)."""
        if getattr(self, 'flat', None) is not None:
            self.flat.zero_grad()
        else:
            self.optimizer.zero_grad(set_to_none=True)

    def _grads_ready(self, world=1, group=None, force=False):
        """After backward: average the gradients over the ranks (ONE all-reduce of one flat tensor) and hand them to the
        optimizer.  Returns the tensors clip_grad_norm_ has to see.  force: issue the collective even in a group of one."""
        if self.flat is None:
            params = list(self.model.parameters())
            if world > 1 or force:
                allreduce_gradients(params, group, force=force)
            return params
        if not self.flat.intact(self.model):
            raise RuntimeError('the model parameters were moved or replaced after initiate_training(): call it again')
        g = self.flat.gradient()               # (gradients that did not come from the model-wide packing gather: by copy)
        if world > 1 or force:
            all_reduce_sum(g, group)
            g.mul_(1.0 / world)
        self.flat.param.grad = g
        return [self.flat.param]

    def _grad_flat(self):
        """After backward: the gradient as ONE vector in parameters() order -- the packing gather's own output on the flat path
        (no copy), a concatenation otherwise (zeros for a parameter without a gradient)."""
        if self.flat is not None:
            return self.flat.gradient()
        return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in self.model.parameters()])

    def _set_grad_flat(self, g):
        """Make the vector g (as _grad_flat's) the gradient the optimiser reads: every .grad becomes a view of it, no unpack
        copies.  Returns the tensors clip_grad_norm_ has to see."""
        if self.flat is not None:
            self.flat.set_grad_vector(g)
            self.flat.param.grad = g
            return [self.flat.param]
        params, off = list(self.model.parameters()), 0
        for p in params:
            p.grad = g[off:off + p.numel()].view_as(p) if p.requires_grad else None       # (frozen: set_trainable)
            off += p.numel()
        return params

    def _clip_and_step(self, clip_params, max_norm):
        """clip_grad_norm_(max_norm) + optimizer.step() (mpnnlstm.py:251, 257); max_norm None: no clipping (:311).  The one
        place every optimiser step goes through: with averaged weights (set_ema) their update follows the step."""
        self._ema_guard()
        grouped = self._grouped if self._groups is not None else None       # (set_param_groups: decay and stash, step, blend)
        if self.flat is not None:
            if self.flat.param.grad is None:
                grouped = None              # (FlatAdam takes no step without a gradient)
            elif self._train_mask is not None:
                self.flat.param.grad.mul_(self._train_mask)         # (set_trainable: the frozen entries are zero from here on)
            if grouped is not None:
                grouped.before(self.optimizer.param_groups[0]['lr'])
            self.optimizer.step(max_norm=max_norm)
        else:
            if max_norm is not None:
                if self._trainable is not None:
                    clip_params = [p for p in clip_params if p.requires_grad]
                torch.nn.utils.clip_grad_norm_(clip_params, max_norm=max_norm)
            if grouped is not None:
                grouped.before(self.optimizer.param_groups[0]['lr'])
            self.optimizer.step()
        if grouped is not None:
            grouped.after()
        if self.ema is not None:
            self.ema.update()

    def _world(self):
        d = torch.distributed
        if self.process_group is not None:
            return d.get_world_size(self.process_group)
        return d.get_world_size() if d.is_available() and d.is_initialized() else 1

    @on_device(lambda self, *a, **k: self.device)
    def train_step(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                   max_norm=10.0, fused=False, pos_weight=None, loss_weights=None, lead_weights=None):
        """zero_grad -> forward -> masked MSE -> backward -> [all-reduce] -> clip_grad_norm_(10) -> Adam
        (mpnnlstm.py:229-257).  x: (T_in, W, H, C) or (B, T_in, W, H, C).  Returns the loss tensor.
        loss_weights / lead_weights: the weighted loss (masked_mse).  fused=True (binary predictors only): the fused binary
        cross-entropy of masked_mse, the loss a captured step runs.  On a binary=True predictor the weights, and pos_weight, the
        weight of the positive class, select the weighted binary cross-entropy (masked_bce)."""
        check_concat_clips(x, concat_layers)
        y, concat_layers = self._first_steps(y, concat_layers)
        lw = self._loss_weights(x, mask, loss_weights, lead_weights, pos_weight)
        self.zero_grad()
        loss = self.forward_loss(x, y, concat_layers, mask, high_interest_region, graph_structure, fused=fused, loss_weights=lw)
        loss.backward()
        self._clip_and_step(self._grads_ready(self._world(), self.process_group), max_norm)
        check_tile_errors()          # (reads the device only when this step issued tile-resident launches; raises on a failed one)
        return loss.detach()

    def _take_grads(self, acc, n):
        """After a micro-batch's backward: acc + n * (its gradient), the gradients dropped (set to None) -- one flat vector on
        the flat path, else a list with one entry per parameter (None: no gradient so far).  acc None: the first micro-batch.
        The sum lives in memory of its own: what autograd hands out is never written to (two .grad fields may alias one buffer,
        ops.unalias, and a gradient may be a view of something a later pass reads)."""
        if self.flat is not None:
            g = self._grad_flat()
            acc = g * n if acc is None else acc.add_(g, alpha=n)
            self.flat.zero_grad()
            return acc
        grads = [p.grad for p in self.model.parameters()]
        if acc is None:
            acc = [None] * len(grads)
        both = [(a, g) for a, g in zip(acc, grads) if a is not None and g is not None]
        if both:
            torch._foreach_add_([a for a, _ in both], [g for _, g in both], alpha=n)
        acc = [g * n if a is None and g is not None else a for a, g in zip(acc, grads)]
        self.optimizer.zero_grad(set_to_none=True)
        return acc

    def _accumulated_backward(self, items, clips, run_loss):
        """zero_grad once, then per micro-batch (x, y, concat) of `items` (of `clips`[i] clips), in order: run_loss(x, y, concat)
        -> loss, backward, sum += n_i * its gradient; at the end sum *= scale, with (n_i, scale) = micro_multipliers(clips), so
        the weights are w_i = n_i * scale = B_i / sum B.  Micro-batches of one clip count have n_i = 1 and scale = 1 / k: the
        arithmetic of the graphed step, bit for bit.  Leaves the result where one backward pass leaves a gradient (the flat
        vector's views on the flat path, .grad per parameter otherwise: what _grads_ready takes) and returns sum_i w_i loss_i,
        formed the same way, detached.  The order of the sum is the order of the micro-batches: the same inputs give the same
        bits.  One micro-batch: its backward, untouched."""
        self.zero_grad()
        if len(items) == 1:
            loss = run_loss(*items[0])
            loss.backward()
            return loss.detach()
        mult, scale = micro_multipliers(clips)
        acc = total = None
        for item, n in zip(items, mult):
            loss = run_loss(*item)
            loss.backward()
            acc = self._take_grads(acc, n)
            total = loss.detach() * n if total is None else total.add_(loss.detach(), alpha=n)
        if self.flat is not None:
            self.flat.set_grad_vector(acc.mul_(scale))
        else:
            torch._foreach_mul_([a for a in acc if a is not None], scale)
            for p, a in zip(self.model.parameters(), acc):
                p.grad = a
        return total.mul_(scale)

    @on_device(lambda self, *a, **k: self.device)
    def accumulated_step(self, batches, mask=None, high_interest_region=None, graph_structure=None, max_norm=10.0, fused=False,
                         pos_weight=None, loss_weights=None, lead_weights=None):
        """Gradient accumulation (beyond the reference): ONE optimiser step from the micro-batches `batches`, a non-empty sequence
        of (x, y) or (x, y, concat_layers), each shaped as train_step takes them; the frames and T_out agree, the clip counts B_i
        may differ.  zero_grad once -> per micro-batch, in order: forward, loss, backward, gradient += w_i * its gradient ->
        [one all-reduce] -> clip_grad_norm_(max_norm) of the ACCUMULATED gradient -> Adam, with w_i = B_i / sum_j B_j
        (micro_weights): the rollout loss is a mean over clips, so this is train_step on the concatenated batch up to rounding,
        while only one micro-batch's activations are ever live.  Returns sum_i w_i loss_i, detached.  The weights are applied as
        integer multiples and ONE scale at the end (micro_multipliers): micro-batches of one shape then give the bits of the
        graphed step (make_graphed_step(accumulate=k)).  With one micro-batch the call is train_step, bit for bit.  The loss weights
        are checked and uploaded once, before the first rollout; an empty `batches`, differing frame shapes and a concat_layers for
        some items only are refused by name before any launch."""
        loss = self.accumulate_gradients(batches, mask, high_interest_region, graph_structure, fused, pos_weight, loss_weights,
                                         lead_weights)
        self._clip_and_step(self._grads_ready(self._world(), self.process_group), max_norm)
        check_tile_errors()
        return loss

    @on_device(lambda self, *a, **k: self.device)
    def accumulate_gradients(self, batches, mask=None, high_interest_region=None, graph_structure=None, fused=False,
                             pos_weight=None, loss_weights=None, lead_weights=None):
        """accumulated_step up to the optimiser: the checks, zero_grad, and every micro-batch's forward, loss and backward.  The
        accumulated gradient is left where one backward pass leaves a gradient, for _grads_ready to take; returns the loss."""
        items = checked_batches('accumulated_step', batches)
        self._check_fused(fused)
        clips = [1 if x.dim() == 4 else x.shape[0] for x, _, _ in items]
        micro_weights(clips)                # (refuses a micro-batch without clips)
        items = [(x, *self._first_steps(y, c)) for x, y, c in items]
        lw = self._loss_weights(items[0][0], mask, loss_weights, lead_weights, pos_weight)
        return self._accumulated_backward(items, clips, lambda x, y, c: self.forward_loss(
            x, y, c, mask, high_interest_region, graph_structure, fused=fused, loss_weights=lw))

    @on_device(lambda self, *a, **k: self.device)
    def truncated_backward(self, x, y, concat_layers, mask, high_interest_region=None, graph_structure=None,
                           truncated_backprop=45, pos_weight=None, loss_weights=None, lead_weights=None):
        """The reference's truncated-BPTT loop (mpnnlstm.py:281-315), quirks included: every chunk re-runs the encoder
        and unrolls ITS steps from the encoder state, `zero_grad` runs per chunk (so only the last chunk's gradient
        survives to optimizer.step()), and the chunk bound is min(start + tb, T_out + 1).  Returns the chunk losses.

        Beyond the reference: a chunk is clamped to the steps that exist, range(max(step - tb, 0), min(step, T_out)).  HEAD
        unrolls range(step - tb, step) as it stands, which leaves [0, T_out) whenever tb does not divide T_out -- the default
        tb = 45 with the notebook's T_out = 10 gives range(-34, 11) and ends in an IndexError at y[unroll_steps] (:308).
        Where HEAD runs (tb divides T_out: ice_exp.py exp 5 / 6) the clamp changes nothing.

        loss_weights / lead_weights: the weighted loss; a chunk takes lead_weights[steps] and divides by that slice's sum (every
        chunk's slice is checked before the first one runs).  pos_weight (binary=True predictors): as in train_step."""
        losses, step = [], 0
        check_concat_clips(x, concat_layers)
        y, concat_layers = self._first_steps(y, concat_layers)
        if y.dim() == 4:
            y = y.unsqueeze(0)
        lw = self._loss_weights(x, mask, loss_weights, lead_weights, pos_weight)
        chunks = []
        while step < self.output_timesteps:
            step = min(step + truncated_backprop, self.output_timesteps + 1)
            steps = range(max(step - truncated_backprop, 0), min(step, self.output_timesteps))
            chunks.append((steps, None if lw is None else lw.chunk(steps)))
        for steps, lwc in chunks:
            self.zero_grad()
            self.model.process_inputs(x, mask=mask, high_interest_region=high_interest_region, graph_structure=graph_structure)
            y_hat, meshes = self.model.unroll_output(steps, y, concat_layers=concat_layers, teacher_forcing_ratio=0, mask=mask,
                                                     high_interest_region=high_interest_region, remesh_every=1)
            if lwc is None:
                loss = masked_mse(y_hat, meshes, y[:, steps.start:steps.stop], mask, self.binary)
            else:
                loss = self._weighted_loss(y_hat, meshes, y[:, steps.start:steps.stop], mask, lwc)
            loss.backward()
            losses.append(loss.detach())
        return losses

    @on_device(lambda self, *a, **k: self.device)
    def make_graphed_step(self, x, y, concat_layers=None, mask=None, high_interest_region=None, max_norm=10.0,
                          warmup=2, graph_structure=None, force_multi=False, accumulate=1, pos_weight=None, loss_weights=None,
                          lead_weights=None):
        """Capture one whole training step in hipGraphs and return `step(x, y, concat) -> loss`.

        The rollout is data dependent (every decoder step re-meshes on its own output), so the capture runs in
        static mode: all node buffers have the worst-case capacity B*W*H and every kernel reads the actual node
        count from device memory -- no host sync, no shape change, ~1.8k launches replayed by one hipGraphLaunch.
        Single process: forward + loss + backward + clip + fused Adam are ONE graph.  Under torch.distributed the
        first graph ends with the gradients packed into one flat buffer; the step is then
        `graph1.replay(); all_reduce(flat); graph2.replay()` with graph2 = average + clip + fused Adam on views of
        that buffer: one collective and three host calls per step.  The `warmup` eager steps are real training steps.
        force_multi: take the multi-rank structure (graph1, all-reduce, graph2) also in a process group of ONE rank -- the
        collective then averages over one rank, i.e. changes nothing, but RCCL, its stream ordering against the two graph
        replays and the capture beside its watchdog thread all run for real (tests/test_gpu_dist.py; bench.py --force-multi).
        loss_weights / lead_weights: the weighted loss (masked_mse); checked and uploaded once, here, and the captured step reads
        the two device arrays -- step(x, y, concat) keeps its signature.
        A binary=True predictor runs the fused binary cross-entropy (masked_mse(fused=True)) in the warm-up steps and in the
        capture alike: torch's BCELoss path indexes with a host mask and cannot be captured.  Given weights or pos_weight it runs
        the weighted binary cross-entropy (masked_bce) instead; pos_weight goes to the kernels by value, so the captured graph
        keeps the value it was captured with -- it is constant for the life of the step object.
        accumulate=k > 1: gradient accumulation.  The returned `step(batches) -> loss` takes a sequence of 1..k items (x, y) or
        (x, y, concat), each of the shape given here, and makes ONE optimiser step from them (_graphed_accumulation); the warm-up
        steps are eager accumulated steps of the one batch given here.  accumulate=1 is the step described above, untouched.
        """
        if check_accumulate(accumulate) > 1:
            return self._graphed_accumulation([(x, y, concat_layers)], accumulate, mask, high_interest_region, max_norm, warmup,
                                              graph_structure, force_multi, pos_weight, loss_weights, lead_weights)
        check_concat_clips(x, concat_layers)
        held = self._held()
        y, concat_layers = self._first_steps(y, concat_layers)
        multi, world = self._capture_setup(force_multi)
        batch = StaticBatch(x, y, concat_layers)
        lw = self._loss_weights(x, mask, loss_weights, lead_weights, pos_weight)

        def fwd_bwd():
            self.zero_grad()
            loss = self.forward_loss(*batch.tensors, mask, high_interest_region, graph_structure, fused=self.binary,
                                     loss_weights=lw)
            loss.backward()
            return loss.detach()

        def warm():
            for _ in range(warmup):
                self.last_warmup_loss = fwd_bwd()        # (a real training step on this batch)
                self._clip_and_step(self._grads_ready(world, self.process_group, force=multi), max_norm)

        side = torch.cuda.Stream()
        warm_then_sync(side, multi, warm)
        graph, graph2 = torch.cuda.CUDAGraph(), None
        ema, averaged = self.ema, self.ema.updates if self.ema is not None else 0
        trainable, train_mask = self._trainable, self._train_mask
        groups, grouped = self._groups, self._grouped if self._groups is not None else None
        self.zero_grad()
        # thread_local: other threads (the RCCL watchdog under torch.distributed) may issue HIP calls meanwhile
        with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
            static_loss = fwd_bwd()
            if multi:                   # the graph ends with the gradients in ONE flat buffer
                flat = self._grad_flat()
            else:
                self._clip_and_step(self._grads_ready(), max_norm)
        self._graph = graph
        if multi:
            clip_params = self._set_grad_flat(flat)
            graph2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph2, stream=side, capture_error_mode='thread_local'):
                flat.mul_(1.0 / world)
                self._clip_and_step(clip_params, max_norm)
        if ema is not None:
            ema.updates = averaged      # (the capture recorded the update's launches without running them; a replay counts)
        watch = TileWatch()

        @on_device(lambda *a, **k: self.device)
        def step(x, y, concat_layers=None):
            self._ema_guard(True, ema)
            self._trainable_guard(trainable)
            self._groups_guard(groups)
            batch.load(x, *self._first_steps(y, concat_layers, held))      # (the horizon of the capture, whatever is set now)
            graph.replay()
            if multi:
                all_reduce_sum(flat, self.process_group)
                graph2.replay()
            if ema is not None:
                ema.advance()
            watch.advance()
            return static_loss
        step.check, step.loss_weights, step.ema, step.horizon = watch.check, lw, ema, held[0]
        step.trainable, step.trainable_mask = trainable, train_mask       # (the graph reads the mask by pointer: it lives with the step)
        step.param_groups, step.grouped = groups, grouped         # (and so do the vectors of the parameter groups)
        return step

    def _capture_setup(self, force_multi):
        """What a captured training step needs before anything runs: whether it takes the multi-rank structure and over how many
        ranks -> (multi, world); static mode; an optimiser whose step counter and learning rate live on the device."""
        import torch.distributed as dist
        if force_multi and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError('force_multi=True needs an initialised torch.distributed process group')
        multi = force_multi or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        world = dist.get_world_size(self.process_group) if multi else 1
        self.model.static_shapes = True
        if not self.optimizer.defaults.get('capturable', False):
            lr = self.optimizer.param_groups[0]['lr']
            assert not self.optimizer.state, 'make_graphed_step must be called before the first optimizer step'
            decay, trainable, groups = None if self.ema is None else self.ema.decay, self._trainable, self._groups
            self.initiate_training(float(lr), self.scheduler.gamma, capturable=True)
            self.set_ema(decay)         # (no step was taken: the average starts with the new optimiser, as it stood)
            self.set_trainable(trainable)       # (and so does the selection of trainable parameters)
            from qtmpnn.groups import as_pairs
            self.set_param_groups(as_pairs(groups))     # (and the parameter groups)
        return multi, world

    def _graphed_accumulation(self, batches, accumulate, mask=None, high_interest_region=None, max_norm=10.0, warmup=2,
                              graph_structure=None, force_multi=False, pos_weight=None, loss_weights=None, lead_weights=None):
        """make_graphed_step(accumulate=k > 1): `step(batches) -> loss` for groups of 1..k micro-batches of ONE shape, that of
        the items of `batches` (1..k of them; the `warmup` steps are eager accumulated steps of exactly these, real training
        steps).  Two graphs, in single-process runs too:

            micro    forward + loss + backward of the static inputs, then acc += flat gradient, loss_acc += loss
            update   acc *= scale[0]; clip + Adam on acc; loss = loss_acc * scale[1]; acc = 0, loss_acc = 0

        and a step is: per item copy-in and micro.replay(); under torch.distributed ONE all_reduce(acc); update.replay().
        `scale` is a device pair that step() sets to (1 / (j * world), 1 / j) for the j items it was given (group_scale), so a
        short last group of an epoch replays the same two graphs.  The items share a shape, so their weights B_i / sum B are 1 / j.
        acc is zero between steps: there is no state beside the optimiser's, and a checkpoint is what it was.  Only one
        micro-batch's activations are ever live.  Stream ordering under torch.distributed as in make_graphed_step
        (warm_then_sync): the warm-up and its collectives on the caller's stream, only the captures on the side stream."""
        k = check_accumulate(accumulate)
        held = self._held()
        items = [(x, *self._first_steps(y, c)) for x, y, c in checked_batches('make_graphed_step', batches)]
        if len(items) > k or any(batch_shapes(item) != batch_shapes(items[0]) for item in items):
            raise ValueError(f'make_graphed_step: batches must be 1..{k} (accumulate) items of one shape, got {len(items)} of shapes '
                             f'{[batch_shapes(item) for item in items]}')
        multi, world = self._capture_setup(force_multi)
        batch = StaticBatch(*items[0])
        lw = self._loss_weights(batch.tensors[0], mask, loss_weights, lead_weights, pos_weight)
        run_loss = lambda x, y, c: self.forward_loss(x, y, c, mask, high_interest_region, graph_structure, fused=self.binary,
                                                     loss_weights=lw)
        dev = batch.tensors[0].device
        n = self.flat.n if self.flat is not None else sum(p.numel() for p in self.model.parameters())
        acc, loss_acc, scale = torch.zeros(n, device=dev), torch.zeros((), device=dev), torch.ones(2, device=dev)

        def warm():
            for _ in range(warmup):
                self.last_warmup_loss = self._accumulated_backward(items, [1] * len(items), run_loss)
                self._clip_and_step(self._grads_ready(world, self.process_group, force=multi), max_norm)

        side = torch.cuda.Stream()
        warm_then_sync(side, multi, warm)
        micro = torch.cuda.CUDAGraph()
        self.zero_grad()
        with torch.cuda.graph(micro, stream=side, capture_error_mode='thread_local'):
            loss = run_loss(*batch.tensors)
            loss.backward()
            acc.add_(self._grad_flat())
            loss_acc.add_(loss.detach())
        clip_params = self._set_grad_flat(acc)          # the optimiser reads acc from here on
        ema, averaged = self.ema, self.ema.updates if self.ema is not None else 0
        trainable, train_mask = self._trainable, self._train_mask
        groups, grouped = self._groups, self._grouped if self._groups is not None else None
        update = torch.cuda.CUDAGraph()
        with torch.cuda.graph(update, stream=side, capture_error_mode='thread_local'):
            acc.mul_(scale[0])
            self._clip_and_step(clip_params, max_norm)
            static_loss = loss_acc * scale[1]
            acc.zero_()
            loss_acc.zero_()
        if ema is not None:
            ema.updates = averaged      # (as in make_graphed_step: one update per call of step, counted there)
        self._graph = micro
        watch, scaled_for = TileWatch(), [None]

        @on_device(lambda *a, **kw: self.device)
        def step(batches):
            self._ema_guard(True, ema)
            self._trainable_guard(trainable)
            self._groups_guard(groups)
            group = [(x, *self._first_steps(y, c, held)) for x, y, c in checked_batches('step', batches)]
            j = len(group)
            if j > k or any(batch_shapes(item) != batch.shapes for item in group):
                raise ValueError(f'step: batches must be 1..{k} items of the captured shape {batch.shapes}, got {j} of '
                                 f'shapes {[batch_shapes(item) for item in group]}')
            for item in group:
                batch.load(*item)
                micro.replay()
            if multi:
                all_reduce_sum(acc, self.process_group)
            if scaled_for[0] != j:
                scale[0].fill_(group_scale(j, world))
                scale[1].fill_(group_scale(j))
                scaled_for[0] = j
            update.replay()
            if ema is not None:
                ema.advance()
            watch.advance(j)
            return static_loss
        step.check, step.loss_weights, step.accumulate, step.graphs, step.ema = watch.check, lw, k, (micro, update), ema
        step.horizon, step.trainable, step.trainable_mask = held[0], trainable, train_mask
        step.param_groups, step.grouped = groups, grouped
        step.buffers = (*batch.tensors, acc, loss_acc, scale)       # (loss_acc is named nowhere else: StaticBatch)
        return step

    @on_device(lambda self, *a, **k: self.device)
    def make_graphed_rollout(self, x, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None):
        """Capture one no-grad inference rollout (predict's loop body for one batch) in a hipGraph and return
        `rollout(x, concat) -> (B, T_out, W, H, 1)` device stack; `rollout.warmup` holds the eager result of the given batch.

        As make_graphed_step: static mode (worst-case capacities, node counts read on the device; the caller restores
        `static_shapes`), one eager warm-up rollout on a side stream -- a real prediction of this batch -- then the capture there.
        Every step's frame is written by one gather launch into its slot of the stack, so a replay ends in ONE host copy.  Host
        state an eager rollout advances is advanced by a replay too: Python's `random` (unroll_output draws once per output step)
        and the attention-dropout seed counter.  In train() mode every replay draws new dropout masks (torch's graph-safe RNG
        for the decoder, the device counter ops.dropout_epoch for attention)."""
        return self._graphed_product(frames_product(x, self.output_timesteps), x, None, concat_layers, mask=mask,
                                     high_interest_region=high_interest_region, graph_structure=graph_structure)

    def _graphed_product(self, reduce, x, y, concat_layers, c0=None, specs=(), **fwd):
        """The capture of one rollout (forward arguments `fwd`) and its product `reduce` (one device tensor, or a tuple of them:
        several products of the one rollout) on static copies of the batch; y is None
        for a product that does not read it, and replay's arguments are then (x, concat), else (x, y, concat).
        specs: the reference specs whose fields the body builds from the static batch (baselines.reference_fields: the torch
        ops are captured with the rollout, so a replay recomputes them) and hands to reduce as its sixth argument; c0: the
        climatology of the launch-state day, for the anomaly references among them -- it then follows concat in replay's
        arguments."""
        check_concat_clips(x, concat_layers)
        held = self._held()
        y, concat_layers = self._first_steps(y, concat_layers)
        self.model.static_shapes = True
        batch = StaticBatch(x, y, concat_layers, c0)
        sx, sy, sc, sc0 = batch.tensors + (None,) * (c0 is None)

        def body():
            with torch.no_grad():
                y_hat, meshes = self.model(sx, concat_layers=sc, teacher_forcing_ratio=0, **fwd)
                if not specs:
                    return reduce(y_hat, meshes, sx, sy, sc)
                return reduce(y_hat, meshes, sx, sy, sc, reference_fields(sx, sc, sc0, specs))
        # (a replay's y and concat are held to the horizon of the capture, whatever is set by then)
        if y is None:
            return self._graphed_inference(body, lambda x, concat_layers=None, c0=None: batch.load(
                x, None, self._first_steps(None, concat_layers, held)[1], c0))
        return self._graphed_inference(body, lambda x, y, concat_layers=None, c0=None: batch.load(
            x, *self._first_steps(y, concat_layers, held), c0))

    def _graphed_one(self, who, reduce, x, y, concat_layers, **fwd):
        """_graphed_product of one product's reduce with the references the maker `who` was asked for (takes_references):
        checked here, before any launch; none asked for is the capture as it was.  With more than two references
        make_graphed_scores(maps=) takes a list of buffers, one per launch (maps_blocks)."""
        references, c0 = self._asked
        if references is None:
            return self._graphed_product(reduce, x, y, concat_layers, **fwd)
        specs = check_references(who, references, concat_layers is not None, self.output_timesteps, tuple(x.shape[-3:-1]))
        if needs_launch_climatology(specs) and c0 is None:
            raise ValueError(f'{who}: references: an anomaly reference needs launch_climatology=, the climatology of the '
                             'launch-state day of the given batch (get_launch_climatology)')
        named = lambda fields: [(spec_name(s), fields[s]) for s in specs]
        return self._graphed_product(lambda y_hat, meshes, x, y, concat, fields: reduce(y_hat, meshes, x, y, concat, named(fields)),
                                     x, y, concat_layers, c0=c0 if needs_launch_climatology(specs) else None, specs=specs, **fwd)

    def _graphed_inference(self, body, load):
        """Warm-up, capture and replay of a no-grad inference body (_graphed_product).  body() reads the
        caller's static inputs and returns a device tensor, or a tuple of them (several products of one rollout); load(...)
        copies a batch into them.  The returned replay(...) loads, replays, advances the host state like an eager rollout and
        returns the capture's result, tensor or tuple; replay.warmup is a copy of the eager warm-up's result, a tuple cloned
        element by element."""
        import random
        T_out = self.output_timesteps
        def warm_body():
            warm = body()
            return tuple(t.clone() for t in warm) if isinstance(warm, tuple) else warm.clone()

        side = torch.cuda.Stream()
        calls0 = ops._ATTN_CALLS[0]
        warm = warm_then_sync(side, False, warm_body)
        calls1 = ops._ATTN_CALLS[0]
        # the capture records launches without running them: whatever host state it advances is put back, and every replay
        # advances it as an eager rollout would
        rstate = random.getstate()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
            result = body()
        random.setstate(rstate)
        ops._ATTN_CALLS[0] = calls1
        TileWatch()             # (the check after the capture only: the replays of an inference capture are not counted)

        @on_device(lambda *a, **k: self.device)
        def replay(*a, **k):
            load(*a, **k)
            graph.replay()
            for _ in range(T_out):
                random.random()
            ops._ATTN_CALLS[0] += calls1 - calls0
            return result
        replay.warmup = warm
        # the graph reads what the body's closure holds (the device maps of extent_product) at every replay: they live as long as
        # the replay does, as make_graphed_step's loss weights do
        replay.body = body
        return replay

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def make_graphed_scores(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                            threshold=0.15, maps=None):
        """make_graphed_rollout with the verification sums in place of the frames: the capture holds the rollout and
        ops.rollout_scores (model, persistence = channel 0 of the last input frame, climatology = concat_layers when given), no
        frame gather.  Returns `scores(x, y, concat) -> (T_out, B, S, 8)` float64 device tensor; `scores.warmup` is the given
        batch's.  maps: a float64 (T_out, S, 8, P) device buffer that the body also adds the batch's per-pixel sums into
        (ops.rollout_score_maps).  The warm-up runs the body once and the capture records it without running, so the given
        batch is added exactly once, and every replay adds its batch once.  With more than two `references` maps is a LIST of
        buffers, one (T_out, 1 + n_i, 8, P) block per launch as maps_blocks makes them; joined_maps(blocks) is the
        (T_out, S, 8, P) array of all sources."""
        return self._graphed_one('make_graphed_scores', sums_product(threshold, maps), x, y, concat_layers, mask=mask,
                                 high_interest_region=high_interest_region, graph_structure=graph_structure)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def make_graphed_reliability(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                                 threshold=0.15, bins=10):
        """make_graphed_scores with the per-bin probability sums in place of the verification sums: the capture holds the
        rollout and ops.rollout_reliability (sources as make_graphed_scores), no frame gather.  Returns
        `reliability(x, y, concat) -> (T_out, B, S, bins, 4)` float64 device tensor; `reliability.warmup` is the given batch's."""
        ops.check_bins('make_graphed_reliability', bins)
        return self._graphed_one('make_graphed_reliability', reliability_product(threshold, bins), x, y, concat_layers, mask=mask,
                                 high_interest_region=high_interest_region, graph_structure=graph_structure)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def make_graphed_fss(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                         threshold=0.15, scales=(1, 3, 5, 9, 17, 33)):
        """make_graphed_scores with the per-scale neighbourhood sums in place of the verification sums: the capture holds the
        rollout and ops.rollout_fss (sources as make_graphed_scores), no frame gather.  Returns
        `fss(x, y, concat) -> (T_out, B, S, len(scales), 5)` int64 device tensor; `fss.warmup` is the given batch's."""
        scales = ops.check_scales('make_graphed_fss', scales)
        return self._graphed_one('make_graphed_fss', fss_product(threshold, scales), x, y, concat_layers, mask=mask,
                                 high_interest_region=high_interest_region, graph_structure=graph_structure)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def make_graphed_edges(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                           threshold=0.15):
        """make_graphed_scores with the ice-edge distance sums in place of the verification sums: the capture holds the rollout
        and ops.rollout_edges (sources as make_graphed_scores), no frame gather.  Returns `edges(x, y, concat) -> (T_out, B, S,
        8)` int64 device tensor; `edges.warmup` is the given batch's."""
        return self._graphed_one('make_graphed_edges', edge_product(threshold), x, y, concat_layers, mask=mask,
                                 high_interest_region=high_interest_region, graph_structure=graph_structure)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def make_graphed_extent(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                            threshold=0.15, regions=None, areas=None):
        """make_graphed_scores with the regional extent sums in place of the verification sums: the capture holds the rollout
        and ops.rollout_extent (sources as make_graphed_scores), no frame gather.  regions / areas: the (W, H) host maps of
        extent(), checked (ops.check_regions) and uploaded here, once.  Returns `extent(x, y, concat) -> (T_out, B, R, 1 + S, 4)`
        float64 device tensor; `extent.warmup` is the given batch's."""
        region_dev, area_dev, R, _ = _extent_maps('make_graphed_extent', regions, areas, x.shape[-3:-1], x.device)
        return self._graphed_one('make_graphed_extent', extent_product(threshold, region_dev, area_dev, R), x, y, concat_layers,
                                 mask=mask, high_interest_region=high_interest_region, graph_structure=graph_structure)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def make_graphed_events(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                            threshold=0.15, kind='breakup', persist=5):
        """make_graphed_scores with the event dates in place of the verification sums: the capture holds the rollout, the
        date scan of every 16 steps and the sums of the date errors (ops.rollout_event_dates: launch state = channel 0 of the
        last input frame, climatology = concat_layers when given), no frame gather.  Returns `events(x, y, concat)` -> one
        int32 device buffer, the int64 sums (B, S1 - 1, 8) followed by the dates (B, S1, P) (split_event_buffer);
        `events.warmup` is the given batch's.  The scan's first launch initialises its state, so a replay needs no memset."""
        return self._graphed_one('make_graphed_events', events_product(threshold, kind, persist), x, y, concat_layers, mask=mask,
                                 high_interest_region=high_interest_region, graph_structure=graph_structure)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def make_graphed_verification(self, x, y, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                                  products=DEFAULT_PRODUCTS):
        """The makers above in one capture: the rollout and the launches of every product of `products` (verify()'s names and
        keywords, checked as verify() checks them, before any launch) as ONE hipGraph.  Returns `verification(x, y, concat)` ->
        the tuple of the products' device tensors in the order given, each what its own maker returns ('predict':
        make_graphed_rollout's stack; 'event_dates': the buffer of make_graphed_events; 'score_maps': the batch's sums, as
        make_graphed_scores(maps=...)); `.warmup` is that tuple for the given batch and `.products` the names.  With 'score_maps'
        the zeroed float64 (T_out, S, 8, P) buffer is allocated here and is `.maps`: the given batch is in it once, and every
        replay adds its batch once.  With more than two references on 'score_maps', `.maps` is the LIST of per-launch blocks
        (maps_blocks) and joined_maps(replay.maps) the (T_out, S, 8, P) array."""
        check_concat_clips(x, concat_layers)
        references, c0 = self._asked
        call = ProductCall(self.output_timesteps, tuple(x.shape[-3:-1]), x.device, concat_layers is not None, True, mask, references)
        made = make_products('make_graphed_verification', products, call)
        specs = product_specs(made.values())
        if needs_launch_climatology(specs) and c0 is None:
            raise ValueError('make_graphed_verification: references: an anomaly reference needs launch_climatology=, the '
                             'climatology of the launch-state day of the given batch (get_launch_climatology)')
        for p in made.values():
            if p.begin is not None:
                p.begin(x)
        replay = self._graphed_product(with_fields(made.values(), [p.reduce(x) for p in made.values()]), x, y, concat_layers,
                                       c0=c0 if needs_launch_climatology(specs) else None, specs=specs,
                                       mask=mask, high_interest_region=high_interest_region, graph_structure=graph_structure)
        replay.products = tuple(made)
        replay.maps = made['score_maps'].maps if 'score_maps' in made else None
        return replay

    @on_device(lambda self, *a, **k: self.device)
    @takes_ema
    @takes_horizon
    @takes_trainable
    @takes_param_groups
    def train(self, loader_train, loader_test, climatology=None, n_epochs=200, lr=0.01, lr_decay=0.95, mask=None,
              high_interest_region=None, truncated_backprop=45, graph_structure=None, use_graph=False, accumulate=1,
              pos_weight=None, test_graph=False, patience=None, min_delta=0.0, restore_best=False, keep_best=None,
              monitor='loss', loss_weights=None, lead_weights=None):
        """The reference's training loop (mpnnlstm.py:186-387).  use_graph=True (beyond the reference) replays the whole training
        step as a hipGraph: one graph is captured per distinct batch shape on first sight (that batch's own update runs eagerly just
        before the capture) and the learning-rate schedule keeps working because the capturable optimizer holds lr in a device
        tensor that StepLR updates in place.  It needs the step to be ONE rollout: truncated_backprop in (0, None), or a truncation
        length that covers all output steps (the default 45 with the notebook's 10: the truncated loop is then a single chunk over
        the whole rollout, without gradient clipping -- mpnnlstm.py:311 is commented out -- and that is what is captured).
        loss_weights (W, H) / lead_weights (T_out,) (beyond the reference): the weighted loss of masked_mse, for the training
        steps and for the test pass alike; checked and uploaded once.  On a binary=True predictor they, and pos_weight (the weight
        of the positive class), select the weighted binary cross-entropy of masked_bce, for the test pass too.
        accumulate=k > 1 (beyond the reference): gradient accumulation.  Consecutive loader items are grouped k at a time and every
        group is ONE optimiser step (accumulated_step; with use_graph=True one graphed accumulated step per batch shape,
        _graphed_accumulation, a group of mixed shapes being stepped eagerly); the last group of an epoch may be short and is
        stepped with what it has.  `running`, `steps` and the Loss/train scalar stay per micro-batch -- every micro-batch of a group
        is entered with the group's loss, the clip-weighted mean of its micro-batches' -- and the scheduler steps per epoch.  The step
        has to be ONE rollout as for use_graph (a truncation that covers all output steps: no clipping, as there): the reference's
        chunk loop zeroes the gradients per chunk, so a real truncation leaves nothing to accumulate and is refused.

        Validation (beyond the reference; with none of the following given the call is what it was, bit for bit).  The test pass
        is the inference loop of predict / verify (_inference) with the loss as its product (loss_product): every batch's loss is
        added as a float64 on the device, in loader order, and the epoch's sum is read ONCE.
        test_graph=True replays the test pass as hipGraphs: one capture per distinct (batch shape, train / eval mode), the first
        batch of a shape being the eager static-mode warm-up, replays from then on and in every later epoch; the captures live
        until train() returns and `static_shapes` is restored after every pass.  A binary=True predictor then runs the fused
        binary cross-entropy, as make_graphed_step does.  It does not need use_graph=True, and use_graph=True does not imply it:
        the default test pass stays eager under use_graph as well.
        patience=k: stop after the first epoch that has seen k epochs without improvement (qtmpnn.validation.best_and_wait:
        an epoch improves when its value is below the best so far by more than min_delta; ties and NaN do not).  The rule reads
        the predictor's WHOLE history, self.test_loss, which checkpoints carry: load_checkpoint + train(patience=k) stops where
        the run that was never interrupted stops.  self.stopped_epoch is the index into that history of the epoch after which
        the run stopped, None if it did not stop early.
        restore_best=True: every improving epoch copies the model's parameters (its state_dict) into device buffers allocated
        before the first batch -- one torch._foreach_copy_, no host traffic -- and after the last epoch they are copied back, in
        place: a make_graphed_step captured earlier keeps working.  THE OPTIMISER'S MOMENTS AND STEP COUNT ARE LEFT AS THEY ARE,
        those of the last epoch.  Only epochs of this call can be restored: if none of them improves on the history the
        predictor came with, the weights stay the last epoch's.
        keep_best=path: every improving epoch calls save_checkpoint(path), after scheduler.step() and after the histories were
        appended, so the file resumes like any checkpoint (its test_loss ends with the best epoch); the format is untouched.
        self.best_epoch / self.best_value (best_and_wait's, indices into the history) are set whenever one of patience,
        restore_best, keep_best or a Monitor is given; every call starts with them, and stopped_epoch, at None, so a call
        without these keywords leaves None and not an earlier call's values.
        monitor='loss', or a qtmpnn.validation.Monitor(products, value, mode): the test pass then makes the monitor's
        verification products (verify()'s names and keywords, checked under the name `train` before the first training batch)
        beside the loss, on the SAME rollout -- one model forward per test batch, with test_graph=True one capture per shape --
        and value(Verification) of every epoch goes to self.monitor_history and the 'Monitor/test' scalar.  patience,
        restore_best and keep_best then read monitor_history in the monitor's mode; self.test_loss stays the loss, and the NaN and
        divergence refusals stay with it.  monitor_history BELONGS TO ONE CALL AND IS NOT CHECKPOINTED: every call with a Monitor
        starts it empty (the next call may monitor another quantity, in another mode), load_checkpoint and initiate_training
        empty it, so a second call and a resumed run start their patience count anew.  A value that is not one finite float is refused
        under `monitor` after the test pass that produced it.
        Each of these keywords is refused by name (TypeError for a wrong type, ValueError for a wrong value) before anything is
        launched and before the optimiser is made.
        ema=decay, ema_eval=True (keywords of this method through takes_ema; beyond the reference): ema=decay is set_ema(decay)
        once the optimiser exists and before the first capture; None leaves the predictor's setting as it is.  With averaged
        weights and ema_eval=True the test pass of every epoch runs inside averaged_weights() -- the loss, a Monitor's products,
        eager or test_graph=True -- so test_loss, monitor_history, patience, best_epoch / best_value and the scalars are those
        of the AVERAGED weights; restore_best snapshots the weights the test pass saw and writes them into the parameters after
        the last epoch; keep_best writes an ordinary checkpoint, live weights and average (format 2).  ema_eval=False only
        maintains the average.  Training itself never reads it: train_loss and the parameters after every epoch are those of the
        run without `ema`, bit for bit.  ema_eval given without averaged weights is refused under its name.
        horizon=None (a keyword of this method through takes_horizon; beyond the reference): a horizon curriculum.  One integer,
        a sequence with one entry per epoch whose last entry holds for every later epoch, or a callable epoch -> integer
        (qtmpnn.horizon.resolve_schedule); the epoch index is len(self.train_loss) at the start of the epoch, the whole history,
        so load_checkpoint + train(horizon=schedule) continues the schedule and ends in the bits of the run that was never
        interrupted.  The training batches of epoch e run under set_horizon(k_e): k_e rollout steps forward and backward, the first
        k_e steps of y, k_e climatology days.  lead_weights keeps the BUILT length and is cut to its first k_e entries, the divisor
        being the one those entries give.  The single-chunk rule of use_graph / accumulate is judged per epoch.  THE TEST PASS
        ALWAYS RUNS AT THE HORIZON IN FORCE WHEN train() WAS CALLED (the built one by default), so test_loss, patience, a Monitor,
        restore_best and keep_best compare like with like across the epochs.  With use_graph=True the captured steps are kept
        per (batch shape, horizon), and those of a horizon the schedule has left are dropped, so that their memory returns.
        The whole schedule of this call's epochs is resolved and checked before the optimiser is made and before any launch;
        an entry above the steps the training loader's y holds is refused on the first batch of its epoch, before its launch.
        Every refusal names `horizon`.  With horizon=None the call is what it was, bit for bit.
        trainable=patterns (a keyword of this method through takes_trainable; beyond the reference): set_trainable(patterns) for
        this call -- applied once the optimiser exists, after initiate_training when the call has to make it, and before the first
        capture; the selection in force before is back when the call returns.  None trains every parameter; left out, the
        predictor's selection stays.  Checked against the parameter names before anything is launched and before the optimiser
        is made; every refusal names `trainable`.
        param_groups=groups (a keyword of this method through takes_param_groups; beyond the reference):
        set_param_groups(groups) for this call, applied and restored as `trainable` is.  None is no setting; left out, the
        predictor's setting stays.  Every refusal names `param_groups`."""
        from qtmpnn import validation
        image_shape = loader_train.dataset.image_shape
        accumulate = check_accumulate(accumulate)
        test_graph = validation.check_flag('test_graph', test_graph)
        patience, min_delta = validation.check_patience(patience), validation.check_min_delta(min_delta)
        restore_best, keep_best = validation.check_flag('restore_best', restore_best), validation.check_keep_best(keep_best)
        monitor = validation.check_monitor(monitor)
        on_loss = isinstance(monitor, str)
        selecting = patience is not None or restore_best or keep_best is not None or not on_loss
        truncate_ = truncated_backprop not in (0, None)
        # the curriculum: the horizons of this call's epochs, by their index into the whole history (None: none asked for)
        first_epoch = len(self.train_loss) if self.training_initiated else 0
        schedule = None if self._horizon_asked is None else resolve_schedule(self._horizon_asked, first_epoch, n_epochs)
        for k in dict.fromkeys([self.output_timesteps] if schedule is None else schedule):       # (every epoch's own horizon)
            single_chunk = truncate_ and truncated_backprop >= k
            at = '' if schedule is None else f' (horizon={k}, epoch {first_epoch + schedule.index(k)})'
            if accumulate > 1 and truncate_ and not single_chunk:
                raise ValueError(f'accumulate: accumulate={accumulate} needs truncated_backprop=0 or >= the output steps, got '
                                 f'truncated_backprop={truncated_backprop} for {k} steps{at} (the truncated loop zeroes the '
                                 'gradients per chunk: only the last chunk of the last micro-batch would reach the optimiser)')
            if use_graph and truncate_ and not single_chunk:
                raise ValueError('use_graph=True needs truncated_backprop=0 or >= the output steps (the truncated loop re-runs the '
                                 f'encoder per chunk){at}')
        made = {}
        if not on_loss:
            made = make_products('train', monitor.products, ProductCall(
                self.output_timesteps, getattr(getattr(loader_test, 'dataset', None), 'image_shape', None), self.device,
                climatology is not None, test_graph, mask))
        if not self.training_initiated:
            self.initiate_training(lr, lr_decay, capturable=use_graph)
        if self._ema_asked[0] is not None:
            self.set_ema(self._ema_asked[0])
        if self._trainable_asked[0]:
            self.set_trainable(self._trainable_asked[1])
        if self._groups_asked[0]:
            self.set_param_groups(self._groups_asked[1])
        averaging = self.averaged_weights if self.ema is not None and self._ema_asked[1] else contextlib.nullcontext
        graphed = {}
        if mask is not None:
            mshape = tuple(host_mask(mask).shape) if not hasattr(mask, 'shape') else tuple(mask.shape)
            assert mshape == tuple(image_shape), f'Mask and image shapes do not match. Got {mshape} and {image_shape}'
        if schedule is None:
            lw = self._loss_weights(None, mask, loss_weights, lead_weights, pos_weight, shape=image_shape)
            weights_at = lambda k: lw
        else:
            # lead_weights has the built length and every pass takes its first entries (no lead_weights: ones, for every horizon)
            full = self._loss_weights(None, mask, loss_weights, lead_weights, pos_weight, shape=image_shape, steps=max(
                [self.built_output_timesteps] + ([] if lead_weights is not None else [self.output_timesteps, *schedule])))
            cut = {k: horizon_weights(full, k) for k in dict.fromkeys([self.output_timesteps, *schedule])}
            lw, weights_at = cut[self.output_timesteps], cut.__getitem__
        # the test pass: the loss of every batch (a capture holds the fused BCE, as a captured step does) and the monitor's products
        test_reduce = loss_product(mask, lw, self.binary, fused=test_graph and self.binary)
        test_graphs = {} if test_graph else None            # (the captures of the test pass, kept across the epochs)
        history = lambda: self.test_loss if on_loss else self.monitor_history       # (what the stopping rule reads)
        mode = 'min' if on_loss else monitor.mode
        state = lambda: list(self.model.state_dict().values())          # (the parameters where they live: views, no copies)
        # what an earlier call left does not speak for this one; a Monitor's history is its call's (another call may monitor another
        # quantity, in another mode), while test_loss goes on across calls
        self.best_epoch = self.best_value = self.stopped_epoch = None
        if not on_loss:
            self.monitor_history = []
        best_state = saved = None
        if restore_best:
            best_state = [torch.empty_like(t) for t in state()]
        st = time.time()
        batch_step = 0
        for epoch in range(n_epochs):
            running, steps = 0.0, 0
            # the epoch's horizon (a curriculum's; else the one in force) holds for its training batches, not for its test pass
            k_e = self.output_timesteps if schedule is None else schedule[epoch]
            under = contextlib.nullcontext() if schedule is None else self.horizon(k_e)
            lw_e = weights_at(k_e)
            single_chunk = truncate_ and truncated_backprop >= k_e
            truncate = truncate_ and not ((use_graph or accumulate > 1) and single_chunk)
            for key in [key for key in graphed if key[1] != k_e]:
                del graphed[key]            # (the captures of a horizon the schedule has left: their memory returns)
            # (the mode is the caller's, as in the reference: train() never calls model.train() / .eval(); ice_exp.py:181, 218 do)
            with under:
                for group in self._micro_groups(loader_train, climatology, accumulate):
                    x, y, concat = group[0]
                    if accumulate > 1:
                        loss = self._group_step(group, accumulate, graphed if use_graph else None, mask, high_interest_region,
                                                graph_structure, None if single_chunk else 10.0, lw_e)
                    elif truncate:
                        loss = self.truncated_backward(x, y, concat, mask, high_interest_region, graph_structure,
                                                       truncated_backprop, loss_weights=lw_e)[-1]
                        # no gradient clipping in this branch (:311 is commented out)
                        self._clip_and_step(self._grads_ready(self._world(), self.process_group), None)
                    elif use_graph:
                        loss = self._first_sight(graphed, group[0], lambda: self.make_graphed_step(
                            x, y, concat, mask=mask, high_interest_region=high_interest_region, warmup=1,
                            graph_structure=graph_structure, max_norm=None if single_chunk else 10.0, loss_weights=lw_e), group[0])
                    else:
                        loss = self.train_step(x, y, concat, mask, high_interest_region, graph_structure, loss_weights=lw_e)
                        if self.debug:      # gradient norms of the two halves of the model (:259-276; clipped like the reference's)
                            for part in ('encoder', 'decoder'):
                                gs = [p.grad.detach().norm() for p in getattr(self.model, part).parameters() if p.grad is not None]
                                self.writer.add_scalar(f'Grad/{part}/grad_norms', torch.stack(gs).norm().item(), batch_step)
                    value = loss.item()
                    for _ in group:             # (one micro-batch, unless accumulate > 1)
                        self.writer.add_scalar('Loss/train', value, batch_step)
                        running += value
                        steps += 1
                        batch_step += 1
            # once per epoch: the graph-replayed steps and the test pass report their tile errors only at the end of the pass
            with averaging():
                running_test, steps_test = self._test_pass(loader_test, climatology, test_reduce, made, test_graph, test_graphs,
                                                           mask=mask, high_interest_region=high_interest_region,
                                                           graph_structure=graph_structure)
            running, running_test = running / (steps + 1), running_test / (steps_test + 1)   # (+1 as the reference, :360-361)
            if np.isnan(running_test):
                raise ValueError('NaN loss :(')
            if running_test > 4:
                raise ValueError('Diverged :(')
            self.writer.add_scalar('Loss/test', running_test, epoch)
            if not on_loss:
                from qtmpnn.verify import Verification
                results = Verification({name: p.finish() for name, p in made.items()}, forecast_sources(climatology is not None))
                monitored = validation.monitored_value(monitor.value(results), epoch)
                self.writer.add_scalar('Monitor/test', monitored, epoch)
            self.scheduler.step()
            self.train_loss.append(running)
            self.test_loss.append(running_test)
            if not on_loss:
                self.monitor_history.append(monitored)
            if selecting:
                self.best_epoch, self.best_value, waited = validation.best_and_wait(history(), min_delta, mode)
                if self.best_epoch == len(history()) - 1:       # this epoch improved
                    if restore_best:
                        with averaging():           # (the weights the test pass saw)
                            torch._foreach_copy_(best_state, state())
                        saved = self.best_epoch
                    if keep_best is not None:
                        self.save_checkpoint(keep_best)
            print(f'{self.experiment_name} | Epoch {epoch} train {self.loss_func_name}: {running:.4f}, '
                  f'test {self.loss_func_name}: {running_test:.4f}, lr: {self.scheduler.get_last_lr()[0]:.4f}, '
                  f'time_per_epoch: {(time.time() - st) / (epoch + 1):.1f}')
            if patience is not None and waited >= patience:
                self.stopped_epoch = len(history()) - 1
                print(f'{self.experiment_name} | Stopped after epoch {epoch}: {waited} epochs without improvement on '
                      f'{self.best_value!r} (epoch {self.best_epoch} of the history)')
                break
        if saved is not None:
            torch._foreach_copy_(state(), best_state)
            print(f'{self.experiment_name} | Restored the parameters of epoch {saved} of the history')
        print(f'Finished in {(time.time() - st) / 60} minutes')
        self.writer.flush()
        self.loss = pd.DataFrame({'train_loss': self.train_loss, 'test_loss': self.test_loss})

    def _test_pass(self, loader, climatology, loss_reduce, made, use_graph, graphed, **fwd):
        """The test pass of one epoch of train(): _inference over `loader` with the loss (loss_reduce, a loss_product) and the
        products `made` ({name: Product}, possibly empty; reset here, collected as _verify collects them) reduced from ONE rollout
        per batch -> (the sum of the batches' losses, the number of batches).  Every batch's float32 loss is added, as a float64
        and in loader order, to one device scalar that is read once after the last batch: the float64 sum of the floats, what a
        Python sum of the .item()s is, to the bit.  graphed: the caller's dict of captures (use_graph), see _inference."""
        products = list(made.values())
        for p in products:
            p.reset()
        begins = [p.begin for p in products if p.begin is not None]
        total, batches = [None], [0]

        def product(x):
            if not products:
                return loss_reduce
            results = with_fields(products, [p.reduce(x) for p in products])
            return lambda *rollout: (loss_reduce(*rollout[:5]), *results(*rollout))

        def consume(result, x):
            loss, results = (result[0], result[1:]) if products else (result, ())
            total[0] = loss.double() if total[0] is None else total[0].add_(loss.double())      # (0.0 + v is v)
            batches[0] += 1
            for p, r in zip(products, results):
                p.collect(r, x)

        self._inference(loader, climatology, product, consume, use_graph, graphed=graphed, specs=product_specs(products),
                        begin=(lambda x: [begin(x) for begin in begins]) if begins else None, **fwd)
        return (0.0 if total[0] is None else total[0].item()), batches[0]

    def _micro_groups(self, loader, climatology, k):
        """The loader's items as train() steps them: lists of k consecutive (x, y, concat), clipped and with their climatology
        (the last list of a pass may be shorter)."""
        group = []
        for x, y, launch_date in loader:
            x, y = self._clip(x), self._clip(y)
            concat = self.get_climatology_array(climatology, launch_date) if climatology is not None else None
            group.append((x, y, concat))
            if len(group) == k:
                yield group
                group = []
        if group:
            yield group

    def _group_step(self, group, accumulate, graphed, mask, high_interest_region, graph_structure, max_norm, lw):
        """One optimiser step of train(accumulate > 1) from the micro-batches `group` -> the group's loss.  graphed: the dict of
        the graphed accumulated steps by batch shape (None: eager).  A group of one shape is captured on first sight of the shape
        -- the group's own update runs eagerly just before the capture -- and replayed from then on; a group of mixed shapes (a
        short last batch of the loader among full ones) is stepped eagerly with the loss a captured step runs."""
        if graphed is None:
            return self.accumulated_step(group, mask, high_interest_region, graph_structure, max_norm=max_norm, loss_weights=lw)
        if any(batch_shapes(item) != batch_shapes(group[0]) for item in group):
            return self.accumulated_step(group, mask, high_interest_region, graph_structure, max_norm=max_norm, fused=self.binary,
                                         loss_weights=lw)
        return self._first_sight(graphed, group[0], lambda: self._graphed_accumulation(
            group, accumulate, mask, high_interest_region, max_norm, 1, graph_structure, loss_weights=lw), (group,))

    def _first_sight(self, graphed, item, capture, args):
        """train(use_graph=True): the step captured for batches shaped like `item` (batch_shapes) under the horizon in force -- the
        key is the pair, a captured step keeps its horizon --, run on *args -> loss.  A key
        is captured on first sight by capture(), whose one warm-up step is that batch's own update, run eagerly just before the
        capture, and whose loss is returned; from then on the shape is replayed."""
        key = (batch_shapes(item), self.output_timesteps)
        if key not in graphed:
            graphed[key] = capture()
            return self.last_warmup_loss
        return graphed[key](*args)

    def _clip(self, t):
        """Loader items are (1, T, W, H, C) like the reference's batch_size=1 loaders, or (B, T, W, H, C)."""
        t = t.to(self.device)
        return t.squeeze(0) if t.shape[0] == 1 else t

    def get_climatology_array(self, climatology, launch_date):
        """Daily normals of the output days (mpnnlstm.py:389-400).  climatology: (Cy, 366, W, H).  launch_date (1,), as the
        reference's batch_size=1 loaders give it: (T_out, W, H, Cy), the reference's.  launch_date (B,) with B > 1 (beyond the
        reference, whose rule reads the first clip's date for a whole batch): (B, T_out, W, H, Cy), entry [c] what the call on
        launch_date[c:c + 1] returns.  T_out is the horizon in force (set_horizon).  The day indices are
        model.utils.output_day_indices per clip, kept per distinct (launch date, T_out) (an epoch meets the dates of the one
        before); they go up as ONE (B, T_out) int64 array and index the normals once."""
        dates = launch_date.numpy()
        if dates.ndim != 1 or len(dates) <= 1:
            return torch.moveaxis(climatology[:, output_day_indices(dates[0], self.output_timesteps)], 0, -1)
        rows = []
        for date in dates:
            key = (date.item(), self.output_timesteps)       # (the steps too: the horizon may differ from call to call)
            if key not in self._output_days:
                self._output_days[key] = output_day_indices(date, self.output_timesteps)
            rows.append(self._output_days[key])
        doys = torch.tensor(rows, dtype=torch.int64).to(climatology.device)
        return torch.moveaxis(climatology[:, doys], 0, -1)

    def get_launch_climatology(self, climatology, launch_date):
        """Daily normals of the launch-state day, the day before the first output day (model.utils.launch_day_index): what
        get_climatology_array is for the output days, by the same rules.  launch_date (1,): (W, H, Cy); launch_date (B,) with
        B > 1: (B, W, H, Cy), entry [c] what the call on launch_date[c:c + 1] returns, ONE (B,) int64 index array and one
        gather.  The index is kept per distinct launch date beside get_climatology_array's (self._launch_days), on first use
        here: a call that asks for no anomaly reference converts no date more than it did."""
        dates = launch_date.numpy()
        if dates.ndim != 1 or len(dates) <= 1:
            return torch.moveaxis(climatology[:, launch_day_index(dates[0])], 0, -1)
        rows = []
        for date in dates:
            key = date.item()
            if key not in self._launch_days:
                self._launch_days[key] = launch_day_index(date)
            rows.append(self._launch_days[key])
        doys = torch.tensor(rows, dtype=torch.int64).to(climatology.device)
        return torch.moveaxis(climatology[:, doys], 0, -1)

    @on_device(lambda self, *a, **k: self.device)
    def predict(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False):
        """Inference over a loader -> (n_clips, T_out, W, H, 1) array (mpnnlstm.py:402-440).

        use_graph=True (beyond the reference) replays every rollout as a hipGraph: each distinct (input shape, climatology shape,
        train / eval mode) is captured once per call (make_graphed_rollout; the first batch of that key is predicted eagerly in
        static mode as the warm-up, and its result is the one returned), later batches copy into the captured inputs, replay and
        make one host copy.  The graphs are dropped and `static_shapes` is restored when the call returns."""
        return self._one('predict', loader, climatology, mask, high_interest_region, graph_structure, use_graph)

    def _inference(self, loader, climatology, product, consume, use_graph, reads_y=True, begin=None, graphed=None, specs=(),
                   **fwd):
        """The inference loop of predict, score, score_maps, reliability, fss, edge_distance, extent, event_dates and verify (all
        through _verify) and of train()'s test pass (_test_pass): per batch begin(x), if given, then one no-grad
        rollout (teacher forcing 0, forward arguments `fwd`) reduced by a reduce(y_hat, meshes, x, y, concat), see frames_product,
        whose result (a tensor, or a tuple of them where several products share the rollout) goes to consume(result, x); x is
        the clipped batch.  product(x) makes the reduce: for every batch of an eager
        call, for every capture of a graphed one, so it must not do what every batch needs (that is begin's).  use_graph: each
        distinct (x shape, y shape where the product reads y, climatology shape, train / eval mode) is captured once per call on
        first sight (_graphed_product); that batch's result is the eager static-mode warm-up's, later batches of the key are
        replays.  The graphs are dropped and `static_shapes` is restored when the call ends, also by an exception of begin or
        consume; the tile error word is read once after the last batch.  graphed: a dict the CALLER owns, for the captures to
        outlive the call (train()'s test pass: captured in the first epoch, replayed in every later one); it is filled here and
        left as it is, and whoever owns it passes the same product, forward arguments and mode with it every time.
        `static_shapes` is restored all the same.
        specs: the reference specs of the products (product_specs).  Their fields are built once per batch, on the device, from
        x, concat and -- for the anomaly references -- the climatology of the launch-state day, which then travels with the
        batch as concat does (get_launch_climatology; part of the captures' key); the reduce gets them as its sixth argument.
        Without specs (every product on its default references) nothing of this happens."""
        self.model.to(self.device)
        with_c0 = needs_launch_climatology(specs)
        own = graphed is None
        graphed, static0 = {} if own else graphed, self.model.static_shapes
        try:
            for x, y, launch_date in loader:
                x, y = self._clip(x), self._clip(y) if reads_y else None
                concat = self.get_climatology_array(climatology, launch_date) if climatology is not None else None
                check_concat_clips(x, concat)
                y = self._first_steps(y)[0]
                if begin is not None:
                    begin(x)
                batch = (x, concat) if y is None else (x, y, concat)
                if with_c0:
                    c0 = self.get_launch_climatology(climatology, launch_date)
                    batch, fwd_c0 = batch + (c0,), dict(c0=c0, specs=specs)
                else:
                    c0, fwd_c0 = None, dict(specs=specs) if specs else {}
                if use_graph:
                    key = batch_shapes(batch) + (self.model.training,)
                    if key not in graphed:
                        graphed[key] = self._graphed_product(product(x), x, y, concat, **fwd_c0, **fwd)
                        result = graphed[key].warmup
                    else:
                        result = graphed[key](*batch)
                else:
                    reduce = product(x)
                    with torch.no_grad():
                        y_hat, meshes = self.model(x, concat_layers=concat, teacher_forcing_ratio=0, **fwd)
                        if specs:
                            result = reduce(y_hat, meshes, x, y, concat, reference_fields(x, concat, c0, specs))
                        else:
                            result = reduce(y_hat, meshes, x, y, concat)
                consume(result, x)
        finally:
            if own:
                graphed.clear()
            self.model.static_shapes = static0
        check_tile_errors(always=True)

    def _verify(self, who, loader, climatology, mask, high_interest_region, graph_structure, use_graph, products):
        """_inference with the products `products` names (make_products: all of them checked and prepared before the first batch)
        on ONE rollout per batch -> ({name: result} in the order given, the call's sources).  Per batch: begin of the products that have one, the
        rollout, every product's reduce on it in order (a tuple of results; with use_graph all of it is one capture per key),
        one collect per product."""
        call = ProductCall(self.output_timesteps, getattr(getattr(loader, 'dataset', None), 'image_shape', None), self.device,
                           climatology is not None, bool(use_graph), mask, self._asked[0])
        made = make_products(who, products, call)
        begins = [p.begin for p in made.values() if p.begin is not None]

        def product(x):
            return with_fields(made.values(), [p.reduce(x) for p in made.values()])

        def consume(results, x):
            for p, result in zip(made.values(), results):
                p.collect(result, x)

        self._inference(loader, climatology, product, consume, use_graph, reads_y=any(p.reads_y for p in made.values()),
                        begin=(lambda x: [begin(x) for begin in begins]) if begins else None, specs=product_specs(made.values()),
                        mask=mask, high_interest_region=high_interest_region, graph_structure=graph_structure)
        # (the call's own sources: the names of its references, which make_products has checked by now)
        sources = forecast_sources(call.with_clim, None if call.references is None else tuple(call.references))
        return {name: p.finish() for name, p in made.items()}, sources

    def _one(self, name, loader, climatology, mask, high_interest_region, graph_structure, use_graph, **options):
        """The method `name`: _verify with that one product."""
        return self._verify(name, loader, climatology, mask, high_interest_region, graph_structure, use_graph, {name: options})[0][name]

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def verify(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False,
               products=DEFAULT_PRODUCTS):
        """Several verification products from ONE rollout per batch -> qtmpnn.verify.Verification (beyond the reference): what
        predict, score, score_maps, reliability, fss, edge_distance, extent and event_dates return, each bit for bit what its own
        method returns with the same arguments, without running the model once per product.

        products: a sequence of those method names (each with its method's defaults), or a mapping name -> dict of that
        method's own keywords (threshold, bins, scales, regions, areas, region_names, kind, persist); one configuration per
        product.  Every product is checked as its own method checks it, under the method's name, before the first batch and
        before any launch; an unknown name, a keyword the method does not take, an empty `products` and a name given twice are
        ValueErrors.  The result holds the products in the order given: `v['fss']`, `v.fss`, `v.products`, `v.sources`.

        score()'s loop and arguments.  Per batch: the rollout once, then every product's launches on it in order, one host copy
        per product.  use_graph=True captures the rollout and all products as ONE hipGraph per distinct batch shape
        (make_graphed_verification).  'predict' is what predict() is in the same mode: eagerly the reference's `unflatten` per
        step, graphed the gathered stack."""
        from qtmpnn.verify import Verification
        return Verification(*self._verify('verify', loader, climatology, mask, high_interest_region, graph_structure, use_graph,
                                          products))

    @on_device(lambda self, *a, **k: self.device)
    def attention_weights(self, x, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None, select=None):
        """The attention coefficients of one no-grad rollout of x (predict's eager forward, teacher forcing 0): the records of
        Seq2Seq.record_attention(select), one per attention convolution call, with PyG's (edge_index, alpha) per record."""
        self.model.to(self.device)
        x = x.to(self.device)
        concat = concat_layers.to(self.device) if concat_layers is not None else None
        check_concat_clips(x, concat)
        concat = self._first_steps(None, concat)[1]
        with torch.no_grad(), self.model.record_attention(select) as records:
            self.model(x, concat_layers=concat, teacher_forcing_ratio=0, mask=mask, high_interest_region=high_interest_region,
                       graph_structure=graph_structure)
        return records

    @on_device(lambda self, *a, **k: self.device)
    def sensitivity(self, x, concat_layers=None, mask=None, high_interest_region=None, graph_structure=None,
                    target=None, leads=None, method='gradient', baseline=None, steps=16):
        """Which input days, channels and pixels a forecast is made from -> qtmpnn.sensitivity.Sensitivity (beyond the
        reference).  x: (T_in, W, H, C) or (B, T_in, W, H, C) on the model's device; concat_layers as in forward_loss.  For
        every clip and every lead time t of `leads` (strictly increasing output steps; None: all) the forecast is summarised as

            J_t = sum_p w_p y_hat[t, p] / sum_p w_p      over the unmasked pixels, w = `target` (W, H) >= 0 (None: ones)

        -- a region, or cell areas (model.utils.cell_area_weights) -- and `.maps[b, l]`, shaped like the clip's input, is

            method='gradient'           dJ_t / dx
                   'gradient_x_input'   dJ_t / dx * (x - baseline)
                   'integrated'         (x - baseline) * mean_k dJ_t / dx at baseline + alpha_k (x - baseline),
                                        alpha_k = (k + 1/2) / steps, k < steps (1..256): integrated gradients, midpoint rule

        baseline: zeros, one (T_in, W, H, C) array or one shaped like x.  `.J` holds J_t at x, `.J_baseline` ('integrated'
        only) J_t at the baseline, so `.completeness()` is what the path integral leaves over.

        THE MESHES ARE HELD FIXED: the maps are the derivative of the rollout on the meshes it built for the unperturbed
        input; the quadtree criterion (which cells split) is a step function of the data and is not differentiated.
        Gradients do flow through everything that carries values across meshes: the pooling of the frames onto the nodes and the
        state transfer between the meshes of consecutive decoder steps.  Every path point of 'integrated' is a clip of its own
        and builds its own meshes, as a batch of different clips does.

        One eager rollout (teacher forcing 0, the caller's train / eval mode) with gradients enabled, then one backward pass
        per lead (torch.autograd.grad on the sum of J_t over the clips: the graph is block diagonal, so every clip gets its
        own map); the seed of a pass is the target summed onto the nodes of step t's mesh, on the device.  The path points of
        'integrated' run as extra clips of batched rollouts, at most 32 clips each.  One host copy ends the call.

        Nothing of the training state changes: for the call's duration no parameter requires a gradient (restored in a
        `finally`; with it the weight-gradient launches do not run), so every param.grad, the flat gradient vector, the
        optimiser, `static_shapes` and the mode are what they were; Python's `random` state and the attention-dropout call
        counter are put back as well.  The recompute mode (set_recompute) is ignored: the lead times' backward passes share one
        plain graph.

        Refusals, by argument name and before any launch: ValueError for target (shape, dtype, NaN / infinite, negative, zero
        sum over the unmasked pixels), leads, method, steps, baseline (also when given with a method that does not use them) and
        x (shape, dtype); NotImplementedError for remesh_input=True models (their encoder assembles its rows without
        autograd); RuntimeError in static mode or inside a graph capture.  There is no use_graph option."""
        from qtmpnn import _lib
        from qtmpnn.sensitivity import CHUNK, Request, Sensitivity
        if not torch.is_tensor(x) or not x.is_floating_point() or x.dim() not in (4, 5):
            raise ValueError('x: a floating-point tensor of shape (T_in, W, H, C) or (B, T_in, W, H, C) is needed, got '
                             + (f'{x.dtype} {tuple(x.shape)}' if torch.is_tensor(x) else type(x).__name__))
        req = Request(x.shape, self.output_timesteps, host_mask(mask), target, leads, method, baseline, steps)
        check_concat_clips(x, concat_layers)
        concat_layers = self._first_steps(None, concat_layers)[1]
        if self.model.remesh_input:
            raise NotImplementedError('sensitivity: remesh_input=True models are not covered (their encoder assembles the rows of '
                                      'every input frame without autograd)')
        if self.model.static_shapes or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError('sensitivity: not in static mode or inside a graph capture (make_graphed_step, make_graphed_rollout, '
                               'predict(use_graph=True)): the backward passes run eagerly on meshes of their own sizes')
        _lib.require_cuda(x, 'x')
        import random
        single = x.dim() == 4
        x5 = (x.unsqueeze(0) if single else x).detach().float()
        B, L = x5.shape[0], len(req.leads)
        dev = x5.device
        concat = None
        if concat_layers is not None:
            concat = concat_layers.to(dev).float()
            concat = concat.unsqueeze(0) if concat.dim() == 4 else concat
        base5 = None
        if req.baseline is not None:
            base5 = torch.from_numpy(req.baseline).to(dev)
            base5 = base5.unsqueeze(0).expand_as(x5) if base5.dim() == 4 else base5
        w = torch.from_numpy(req.target).to(dev).reshape(-1)                       # (P,), zero under the mask
        fwd = dict(mask=mask, high_interest_region=high_interest_region, graph_structure=graph_structure)

        def rollout(clips, conc, grads):
            """One rollout of `clips` (n, T_in, W, H, C) -> (J (n, L) float64, maps (n, L, T_in, W, H, C) or None)."""
            n = clips.shape[0]
            leaf = clips.clone().requires_grad_(grads)
            with torch.enable_grad() if grads else torch.no_grad():
                y_hat, meshes = self.model(leaf, concat_layers=conc, teacher_forcing_ratio=0, **fwd)
            J = torch.empty(n, L, dtype=torch.float64, device=dev)
            maps = torch.empty(n, L, *clips.shape[1:], device=dev) if grads else None
            for l, t in enumerate(req.leads):
                out, mesh = y_hat[t], meshes[t]
                with torch.no_grad():
                    frame = ops.gather_pixels(out.detach()[:, :1], mesh).view(n, -1)
                    J[:, l] = (frame.double() * w.double()).sum(dim=1) / req.sum_w
                    if grads:       # dJ_t / d(node output): the target summed onto the nodes of this step's mesh
                        seed = ops.pool_image(w.view(1, 1, -1, 1).expand(n, 1, -1, 1), mesh, False)[0] / req.sum_w
                if grads:
                    maps[:, l] = torch.autograd.grad((out[:, :1] * seed).sum(), leaf, retain_graph=l + 1 < L)[0]
            return J, maps

        params = list(self.model.parameters())
        flat = self.model.__dict__.get('_flat_params')
        if flat is not None:
            params.append(flat.param)           # (a packed model: the optimiser's one tensor over the same storage)
        required = [p.requires_grad for p in params]
        rstate, calls, mode, cut = random.getstate(), ops._ATTN_CALLS[0], self.model.recompute, self.model.encoder_cut
        try:
            self.model.set_recompute(None)          # (several backward passes over one graph: the plain rollout's)
            self.model.set_encoder_cut(False)       # (the maps are gradients THROUGH the encoder, whatever is trained)
            for p in params:
                p.requires_grad_(False)
            self.model.to(self.device)
            Jb = None
            if req.method == 'integrated':
                start = base5 if base5 is not None else torch.zeros_like(x5)
                delta = x5 - start
                alphas = (torch.arange(req.steps, device=dev, dtype=torch.float32) + 0.5) / req.steps
                # the clips of the path, clip-major: point (b, k) = baseline_b + alpha_k (x_b - baseline_b); then the two ends
                points = (start.unsqueeze(1) + alphas.view(1, -1, 1, 1, 1, 1) * delta.unsqueeze(1)).reshape(-1, *x5.shape[1:])
                ends = torch.cat([x5, start])
                pc = ec = None
                if concat is not None:
                    pc = concat.unsqueeze(1).expand(-1, req.steps, *concat.shape[1:]).reshape(-1, *concat.shape[1:])
                    ec = torch.cat([concat, concat])
                chunks = lambda clips, conc, grads: [rollout(clips[a:a + CHUNK], None if conc is None else conc[a:a + CHUNK], grads)
                                                     for a in range(0, clips.shape[0], CHUNK)]
                Js = torch.cat([j for j, _ in chunks(ends, ec, False)])
                J, Jb = Js[:B], Js[B:]
                grads = torch.cat([g for _, g in chunks(points, pc, True)])
                maps = grads.view(B, req.steps, L, *x5.shape[1:]).mean(dim=1) * delta.unsqueeze(1)
            else:
                J, maps = rollout(x5, concat, True)
                if req.method == 'gradient_x_input':
                    maps = maps * ((x5 - base5) if base5 is not None else x5).unsqueeze(1)
            # one host copy: [J | J_baseline] as float64 words in front of the float32 maps
            nj = J.numel() * (2 if Jb is not None else 1)
            buf = torch.empty(2 * nj + maps.numel(), dtype=torch.float32, device=dev)
            buf[:2 * nj].view(torch.float64).copy_(torch.cat([J.reshape(-1)] + ([Jb.reshape(-1)] if Jb is not None else [])))
            buf[2 * nj:].copy_(maps.reshape(-1))
            host = buf.cpu().numpy()
        finally:
            for p, r in zip(params, required):
                p.requires_grad_(r)
            random.setstate(rstate)
            ops._ATTN_CALLS[0] = calls
            self.model.set_recompute(mode)
            self.model.set_encoder_cut(cut)
        check_tile_errors()
        Js = host[:2 * nj].view(np.float64).reshape(-1, B, L)
        return Sensitivity(host[2 * nj:].reshape(B, L, *x5.shape[1:]).copy(), req.leads, req.method, req.target, Js[0].copy(),
                           Js[1].copy() if Jb is not None else None)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def score(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False,
              threshold=0.15):
        """Forecast verification over a loader -> qtmpnn.score.Scores (beyond the reference, whose score() is empty; the numbers
        are those its ice_results.py computes from predict()'s array: masked RMSE and ice / no-ice accuracy per launch date and
        lead time, for the model and the baselines).

        predict()'s loop and arguments, with the loader's y: every batch leaves eight sums per (lead time, clip, source) on the
        device (ops.rollout_scores: the head's outputs read through the labels, no frame is built) and makes one host copy of
        them.  Sources: 'model', 'persistence' (channel 0 of the last input frame at every lead time) and, with `climatology`,
        'climatology' (the daily normals the decoder gets).  `threshold` separates ice from no ice (strict >); with binary=True
        the outputs are probabilities and a caller passes 0.5.  use_graph=True replays rollout + sums as one hipGraph per
        distinct batch shape, as predict(use_graph=True) does (make_graphed_scores).  `.maps` of the result is None: score_maps()
        is this call with the per-pixel maps as well.
        references= (a keyword of this and every other product method, of verify and of the makers: takes_references) names the
        reference forecasts in place of that default pair: a sequence of 'persistence', 'climatology', 'anomaly_persistence' or
        qtmpnn.baselines.AnomalyPersistence objects; the sources are then ('model',) + their names in the order given, and more
        than two cost one more launch of the same kernels per pair."""
        return self._one('score', loader, climatology, mask, high_interest_region, graph_structure, use_graph,
                         threshold=threshold)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def score_maps(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False,
                   threshold=0.15):
        """score() with per-pixel maps from the same pass: the returned Scores has the same `.sums`, bit for bit, and `.maps`, a
        qtmpnn.score.ScoreMaps of (T_out, S, 8, W, H) float64: the eight sums per lead time, source and pixel, over every clip
        of the loader (where the ice edge is over- or under-forecast, where the model beats climatology; `.pooled(weights=...)`
        for cell areas or a region).  The first batch allocates the zeroed device buffer, every batch adds into it right after
        its sums (ops.rollout_score_maps; inside the capture with use_graph=True) and one host copy follows the last batch.
        Every batch must have the first one's frame shape."""
        return self._one('score_maps', loader, climatology, mask, high_interest_region, graph_structure, use_graph,
                         threshold=threshold)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def reliability(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False,
                    threshold=0.15, bins=10):
        """Probability verification over a loader -> qtmpnn.reliability.Reliability (beyond the reference): every source's value
        is read as a forecast probability of the event `y > threshold` (strict) -- the probabilities of a binary=True head
        (pass threshold=0.5: a 0/1 truth is then the event itself), or a concentration in [0, 1] read as a probability of ice --
        and binned into `bins` (2..32) equal bins of [0, 1]; values below 0 and above 1 fall into the end bins.  The result
        gives the reliability diagram, sharpness, Brier score with its decomposition, skill against climatology and the ROC.

        score()'s loop, arguments and sources: every batch leaves four sums per (lead time, clip, source, bin) on the device
        (ops.rollout_reliability: the head's outputs read through the labels, no frame is built) and makes one host copy of
        them.  use_graph=True replays rollout + sums as one hipGraph per distinct batch shape (make_graphed_reliability)."""
        return self._one('reliability', loader, climatology, mask, high_interest_region, graph_structure, use_graph,
                         threshold=threshold, bins=bins)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def fss(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False,
            threshold=0.15, scales=(1, 3, 5, 9, 17, 33)):
        """Neighbourhood verification over a loader -> qtmpnn.fss.FSS (beyond the reference): the Fractions Skill Score
        (Roberts & Lean 2008) of every source at every window size of `scales` (up to 8 odd sizes in 1..33, increasing).  A
        pixel is compared through the number of ice pixels (`value > threshold`, strict) in the window around it, so an ice
        edge that sits two pixels off is charged for those two pixels and not, as in score()'s table, as a miss and a false
        alarm.  The result gives the score per lead time and scale, the skill against persistence and the smallest useful scale.

        score()'s loop, arguments and sources: every batch leaves five integers per (lead time, clip, source, scale) on the
        device (ops.rollout_fss: the head's outputs read through the labels, no frame is built) and makes one host copy of
        them.  use_graph=True replays rollout + sums as one hipGraph per distinct batch shape (make_graphed_fss)."""
        return self._one('fss', loader, climatology, mask, high_interest_region, graph_structure, use_graph,
                         threshold=threshold, scales=scales)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def edge_distance(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False,
                      threshold=0.15):
        """Ice-edge verification over a loader -> qtmpnn.edges.EdgeDistance (beyond the reference): how far, in pixels, the
        forecast ice edge lies from the observed one, per launch date, lead time and source -- the average ice-edge displacement,
        the modified Hausdorff and Hausdorff distances (Dukhovskoy et al. 2015, Melsom et al. 2019) and the RMS distance.  The
        edge of a field is its ice pixels (`value > threshold`, strict) with an open-water 4-neighbour; coasts, masked pixels and
        the frame border make no edge.  Frames of at most 256 x 256.

        score()'s loop, arguments and sources: every batch leaves eight integers per (lead time, clip, source) on the device
        (ops.rollout_edges: the head's outputs read through the labels, no frame is built) and makes one host copy of them.
        use_graph=True replays rollout + sums as one hipGraph per distinct batch shape (make_graphed_edges)."""
        return self._one('edge_distance', loader, climatology, mask, high_interest_region, graph_structure, use_graph,
                         threshold=threshold)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def extent(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False,
               threshold=0.15, regions=None, areas=None, region_names=None):
        """Sea-ice extent, sea-ice area and the integrated ice-edge error over a loader -> qtmpnn.extent.Extent (beyond the
        reference): per launch date, lead time and region the observed and forecast extent (the area of the pixels with `value >
        threshold`, strict) and ice area (the area-weighted sum of the values), and the over- and under-forecast areas O and U
        from which the result forms IIEE = O + U, the absolute extent error |O - U| and the misplacement error 2 min(O, U)
        (Goessling et al. 2016) per forecast.  regions: a (W, H) integer map, region index per pixel, negative for none, at most
        32 regions (None: one region of every pixel); areas: a (W, H) map of cell areas, finite and non-negative, in whose
        unit the results are (model.utils.cell_area_weights for a latitude-longitude grid; None: 1, i.e. pixel counts);
        region_names: a name per region index.  The maps are checked and uploaded once, before the first batch.

        score()'s loop, arguments and sources: every batch leaves (1 + S) * 4 sums per (lead time, clip, region) on the device
        (ops.rollout_extent: the head's outputs read through the labels, no frame is built) and makes one host copy of them.
        use_graph=True replays rollout + sums as one hipGraph per distinct batch shape (make_graphed_extent)."""
        return self._one('extent', loader, climatology, mask, high_interest_region, graph_structure, use_graph,
                         threshold=threshold, regions=regions, areas=areas, region_names=region_names)

    @on_device(lambda self, *a, **k: self.device)
    @takes_references
    def event_dates(self, loader, climatology=None, mask=None, high_interest_region=None, graph_structure=None, use_graph=False,
                    threshold=0.15, kind='breakup', persist=5):
        """Break-up / freeze-up dates over a loader -> qtmpnn.events.EventDates (beyond the reference): per clip, source and
        pixel the first output step from which the pixel is no ice (kind='breakup') or ice ('freezeup') for `persist`
        consecutive steps, ice = value > threshold (strict); -1 where there is no such step or the pixel is in that state at
        launch already (channel 0 of the last input frame), -2 where the pixel is masked or has no node at some step.
        Sources: 'observed' (the loader's y), 'model' and, with `climatology`, 'climatology'; `.sums` compares the forecast
        sources' dates with the observed ones (hits, false alarms, misses, date errors in days).

        score()'s loop and arguments: the dates are scanned on the device along the rollout's time axis (the head's outputs
        read through every step's labels, no frame is built; ops.rollout_event_dates) and every batch makes one host copy of
        dates and sums.  use_graph=True replays rollout + scan + sums as one hipGraph per distinct batch shape
        (make_graphed_events)."""
        return self._one('event_dates', loader, climatology, mask, high_interest_region, graph_structure, use_graph,
                         threshold=threshold, kind=kind, persist=persist)

