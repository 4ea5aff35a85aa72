"""The averaged weights restated: a float64 model of qtmpnn.ema.WeightEMA over a list of recorded iterates, the error bound a
float32 run of its op sequence has to keep, a checker, and a float32 form with the same statements (the yardstick: clean it passes
the checker, and every tampered form of it must fail).  Not a test module; test_ema_host.py and test_gpu_ema.py import it.

The op sequence (WeightEMA's docstring), d = decay, t = 1, 2, ...:

    s_t = fl(fl(d^ * s_{t-1}) + fl(a^ * p_t)),  d^ = fp32(d), a^ = fp32(1 - d)        s_0 = 0
    m_t = s_t / c^,  c^ = fp32(1 - d ** t)  (1 - d ** t formed in float64)

THE BOUND, from the float64 values alone.  u = 2^-24.  Every term of the update passes K_UPDATE = 3 roundings: its constant (d^
or a^), its product, and the sum -- (1 + u)^3 - 1 <= g3 = 3u / (1 - 3u) on either term.  With FMA contraction the second product
is not rounded (2 roundings on that term, 3 on the other), so 3 bounds both forms.  With e_{t-1} >= |s^_{t-1} - s_{t-1}|:

    s^_t = d s^_{t-1} (1 + th) + (1 - d) p_t (1 + th'),  |th|, |th'| <= g3
    e_t  = d (1 + g3) e_{t-1} + g3 (d |s_{t-1}| + (1 - d) |p_t|) + 3 * 2^-149          (the last term: results below 2^-126)

which is the issue's e_t = d e_{t-1} + k u (d |s_{t-1}| + (1 - d) |p_t|) with k = 3 and the second-order terms kept.  The
average passes K_DEBIAS = 3 more: the divisor's rounding to fp32, and either one division (2 in all) or, where the divisor is a
host scalar and the kernel multiplies by its rounded reciprocal, the reciprocal and the product (3 in all):

    |m^_t - m_t| <= (e_t (1 + g3) + g3 |s_t|) / c + 2^-149

d = 0 and d = 0.5 have exact constants and the bound does not use that; the tests ask d = 0 for the iterate itself, exactly."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
K_UPDATE = 3        # constant, product, sum on either term (FMA: 2 on the contracted term)
K_DEBIAS = 3        # fp32(divisor) + division, or + reciprocal + product
gamma = lambda k: k * U / (1.0 - k * U)

TAMPERS = ('no_debias', 'swapped', 'pre_step', 'count_off', 'init_params')


def model64(iterates, d):
    """The float64 recurrence over `iterates` (arrays of one shape, p_1..p_T, any float dtype) -> per t a dict with the shadow
    's', the average 'm' and their bounds 'e_s', 'e_m' (arrays of that shape)."""
    d = float(d)
    g, gd = gamma(K_UPDATE), gamma(K_DEBIAS)
    s = np.zeros(np.shape(iterates[0]), np.float64)
    e = np.zeros_like(s)
    out = []
    for t, p in enumerate(iterates, 1):
        p = np.asarray(p, np.float64)
        e = d * (1.0 + g) * e + g * (d * np.abs(s) + (1.0 - d) * np.abs(p)) + K_UPDATE * TINY
        s = d * s + (1.0 - d) * p
        c = 1.0 - d ** t
        out.append({'s': s, 'm': s / c, 'e_s': e, 'e_m': (e * (1.0 + gd) + gd * np.abs(s)) / c + TINY})
    return out


def form32(iterates, d, start=None, tamper=None):
    """The same statements in float32 (numpy, no contraction) -> [(s_t, m_t)] per t.  tamper: None, or one of TAMPERS --
        no_debias     m_t = s_t
        swapped       d and 1 - d change places in the update
        pre_step      the update reads the parameters of before the step (p_{t-1}; `start` is p_0)
        count_off     the divisor is that of t + 1 updates
        init_params   s_0 = p_0 (`start`) while m_t is still divided by 1 - d ** t"""
    assert tamper is None or tamper in TAMPERS
    f = np.float32
    dd, aa = (f(1.0 - d), f(d)) if tamper == 'swapped' else (f(d), f(1.0 - d))
    ps = [np.asarray(p, f) for p in iterates]
    if tamper in ('pre_step', 'init_params'):
        start = np.asarray(start, f)
    s = start.copy() if tamper == 'init_params' else np.zeros_like(ps[0])
    out = []
    for t, p in enumerate(ps, 1):
        if tamper == 'pre_step':
            p = start if t == 1 else ps[t - 2]
        s = dd * s + aa * p
        c = f(1.0 - float(d) ** (t + 1 if tamper == 'count_off' else t))
        out.append((s, s if tamper == 'no_debias' else s / c))
    return out


def worst(got_s, got_m, ref):
    """The largest |got - model| / bound over the elements, of the shadow and of the average, against one entry of model64
    (a value <= 1 keeps the bound).  got_*: arrays or None (not looked at)."""
    ratio = lambda got, want, bound: 0.0 if got is None else float(np.max(np.abs(np.asarray(got, np.float64) - want) / bound))
    return ratio(got_s, ref['s'], ref['e_s']), ratio(got_m, ref['m'], ref['e_m'])


def holds(got_s, got_m, ref):
    ws, wm = worst(got_s, got_m, ref)
    return ws <= 1.0 and wm <= 1.0


def walk(seed, shape, steps, step=0.01):
    """Iterates of a run that moves: p_0 (the start weights) ~ 0.1 N(0, 1) and p_t = p_{t-1} + step N(0, 1), float32 ->
    (p_0, [p_1..p_steps])."""
    rng = np.random.default_rng(seed)
    p0 = (0.1 * rng.standard_normal(shape)).astype(np.float32)
    ps, p = [], p0
    for _ in range(steps):
        p = (p + step * rng.standard_normal(shape)).astype(np.float32)
        ps.append(p)
    return p0, ps
