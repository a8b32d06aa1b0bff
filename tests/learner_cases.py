"""Cases and float64 references shared by tests/test_learner_cases.py (no GPU: the references against the oracle and the
library formulation, the cases against wrong variants) and tests/test_learner_kernels_gpu.py (the kernels): the glue kernels
of the update (csrc/learner.hip: TD epilogue, Adam, Gumbel top-k, replay scatter / gather, logit extrema) and the two arg-max
heads of csrc/qnet.hip.  numpy only.

Every `*_ref` is a plain float64 restatement of what include/stackrl_qnet.h states, every `*_f32` the same expressions in
float32 on the host.  The scalars the ABI takes as `float` are rounded to float32 when a case is built (`f32s`), so that a
reference evaluates the header's formula at the arguments the kernel receives.

Tolerances.  Integer, index, byte and copied outputs are exact.  A float32 arithmetic output is held to the float64 reference
within C * 2^-24 * (a scale built from the reference's operand magnitudes); every C below is 4 x the largest error of the
float32 host restatement against float64 over this module's own cases, measured on the CPU by `measure_*` (the margin
tests/test_train_conv_gpu.py uses for "float32 on the host against float64"); tests/test_learner_cases.py re-measures and
holds the recorded figures.  No figure comes from a kernel."""
import numpy as np

U = 2.0 ** -24          # half a float32 ulp of 1: the unit of every bound
F = np.float32
NEG_INF = -np.inf


def f32s(x):
  """A Python float holding the float32 nearest to x (what a `float` argument of the ABI receives)."""
  return float(np.float32(x))


# ================================================================================================ arg-max (both heads, TD)
def argmax_ref(rows):
  """Lowest index of each row's maximum; -inf entries take part like any value (a row of nothing but -inf gives 0), NaN
  entries are skipped (a row of nothing but NaN gives 0)."""
  x = np.asarray(rows, np.float64)
  x = np.where(np.isnan(x), -np.inf, x)
  return np.argmax(x, axis=-1)                  # numpy: the first of equal maxima


HEAD_AS = (1, 5, 255, 257, 2401)
HEAD_ROW_KINDS = ('random', 'some -inf', 'below -3e38', 'all -inf', 'one finite', 'tie', 'NaN and finite', 'NaN and -inf',
                  'all NaN')


def head_rows(A, seed=0):
  """[(kind, row float32 [A])]: the rows of HEAD_ROW_KINDS that exist at A actions."""
  rng = np.random.RandomState(1000 + A + seed)
  out = [('random', rng.normal(size=A).astype(F))]
  r = rng.normal(size=A).astype(F); r[rng.rand(A) < 0.4] = NEG_INF; r[0] = NEG_INF; r[A - 1] = 0.5
  out.append(('some -inf', r))
  r = np.full(A, NEG_INF, F); r[::2] = F(-3.2e38); r[A // 2] = F(-3.1e38)            # finite, all below the old start value
  out.append(('below -3e38', r))
  out.append(('all -inf', np.full(A, NEG_INF, F)))
  r = np.full(A, NEG_INF, F); r[(2 * A) // 3] = F(-1.5)
  out.append(('one finite', r))
  if A >= 2:
    r = rng.normal(size=A).astype(F); r[A // 3] = r[A - 1] = F(9.0)
    out.append(('tie', r))
    r = rng.normal(size=A).astype(F); r[0] = np.nan; r[A // 2] = np.nan if A > 2 else r[A // 2]
    out.append(('NaN and finite', r))
    r = np.full(A, NEG_INF, F); r[0] = np.nan
    out.append(('NaN and -inf', r))
  out.append(('all NaN', np.full(A, np.nan, F)))
  return out


# ================================================================================================ Adam
ADAM_BETAS = ((0.9, 0.999), (0.95, 0.95))
ADAM_NS = (1, 3, 4, 1023, 1024, 1027)       # no vector group; tail only; no tail; groups = n / 4 + 1 fill a block; one over; tail of 3
ADAM_STEPS = 6
ADAM_LR = 1e-3
ADAM_EPS = 1e-7


def adam_case(n, betas, seed=0):
  """Parameters at magnitude 1e-3 (a float32 ulp of p is far below a step of lr = 1e-3), gradients redrawn every step over
  10^[-8, 1] with random signs: a band of them has sqrt(v) near eps."""
  rng = np.random.RandomState(7 * n + int(1000 * betas[0]) + seed)
  p = (rng.normal(size=n) * 1e-3).astype(F)
  grads = [(rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-8, 1, size=n)).astype(F) for _ in range(ADAM_STEPS)]
  return dict(p=p, m=np.zeros(n, F), v=np.zeros(n, F), grads=grads, lr=f32s(ADAM_LR), b1=f32s(betas[0]), b2=f32s(betas[1]),
              eps=f32s(ADAM_EPS))


def adam_ref(p, m, v, grads_per_step, lr, b1, b2, eps, dtype=np.float64, variant=None):
  """The header's Keras Adam from the state {0, 1, 1, 0}: a list, one entry per step, of dict(p, m, v, state) with state =
  [t, b1^t, b2^t, lr_t].  dtype float32 gives the host restatement in the kernel's precision.  `variant` names a WRONG
  formula (tests/test_learner_cases.py holds the cases against them)."""
  T = dtype
  p, m, v = (np.array(a, dtype=T) for a in (p, m, v))
  lr, b1, b2, eps, one = T(lr), T(b1), T(b2), T(eps), T(1)
  if variant == 'betas swapped':
    b1, b2 = b2, b1
  t, p1, p2 = T(0), T(1), T(1)
  out = []
  for g in grads_per_step:
    g = np.asarray(g, dtype=T)
    t = t + one; p1 = p1 * b1; p2 = p2 * b2
    lrt = lr * np.sqrt(one - p2) / (one - p1)
    m = m + (g - m) * (one - b1)
    v = v + (g * g - v) * (one - b2)
    if variant == 'eps after the bias correction':          # torch.optim.Adam: lr mhat / (sqrt(vhat) + eps)
      p = p - (lr / (one - p1)) * m / (np.sqrt(v) / np.sqrt(one - p2) + eps)
    elif variant == 'eps inside the square root':
      p = p - (lrt * m) / np.sqrt(v + eps)
    else:
      p = p - (lrt * m) / (np.sqrt(v) + eps)
    out.append(dict(p=p.copy(), m=m.copy(), v=v.copy(), state=np.array([t, p1, p2, lrt], dtype=T)))
  return out


def adam_scales(case, ref):
  """Per step: the magnitudes the bounds are relative to.  m is a convex combination of the gradients so far and v of their
  squares: max |g| and max g^2 over the steps so far, per element.  p: |p0| plus the sizes of all steps so far.  state: b^t
  is t float32 products (t b^t); lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) carries the rounding of b^t amplified by
  b^t / (1 - b^t)."""
  sm = np.zeros_like(ref[0]['m']); sv = np.zeros_like(sm); sp = np.abs(np.asarray(case['p'], np.float64))
  prev = np.asarray(case['p'], np.float64)
  out = []
  for g, r in zip(case['grads'], ref):
    g = np.asarray(g, np.float64)
    sm = np.maximum(sm, np.abs(g)); sv = np.maximum(sv, g * g); sp = sp + np.abs(r['p'] - prev); prev = r['p']
    t, p1, p2, lrt = r['state']
    ss = np.array([0.0, t * p1, t * p2, lrt * (1 + t * p2 / (1 - p2) + t * p1 / (1 - p1))])
    out.append(dict(m=sm.copy(), v=sv.copy(), p=sp.copy(), state=ss))
  return out


# C per beta pair and step 1..ADAM_STEPS = 4 x the float32 host restatement's largest error / (2^-24 scale) over ADAM_NS.
# measured (float32 host vs float64), in units of 2^-24 scale; bound = 4 x measured (ADAM_C)
ADAM_MEASURED = {
    (0.9, 0.999): {
        'm': (0.0952, 0.245, 0.307, 0.352, 0.314, 0.35),
        'v': (0.00194, 0.00378, 0.00609, 0.0039, 0.00448, 0.00467),
        # p carries lr_t's rounding: 1 - b2^t = 0.002 at t = 2 is known to 2^-24 / 0.002 only, 3e-5 of the step
        'p': (3.72, 54.2, 108, 84.1, 72.2, 71.1),
        'state': (0.000438, 0.149, 0.23, 0.103, 0.0804, 0.115),
    },
    (0.95, 0.95): {
        'm': (0.0472, 0.163, 0.137, 0.172, 0.189, 0.21),
        'v': (0.0816, 0.157, 0.18, 0.213, 0.254, 0.205),
        'p': (3.28, 4.4, 4.28, 3.95, 3.92, 3.9),
        'state': (0.00656, 0.0556, 0.0259, 0.122, 0.0286, 0.114),
    },
}
ADAM_C = {b: {k: tuple(4.0 * x for x in v) for k, v in d.items()} for b, d in ADAM_MEASURED.items()}


def adam_errors(got, ref, scales):
  """Largest |got - ref| / (2^-24 scale) per quantity for one step (scale 0: the values must be equal, else inf)."""
  out = {}
  for k in ('m', 'v', 'p', 'state'):
    d = np.abs(np.asarray(got[k], np.float64) - ref[k]); s = U * scales[k]
    with np.errstate(divide='ignore', invalid='ignore'):
      e = np.where(d == 0, 0.0, d / s)
    out[k] = float(e.max())
  return out


def measure_adam():
  worst = {b: {k: [0.0] * ADAM_STEPS for k in ('m', 'v', 'p', 'state')} for b in ADAM_BETAS}
  for betas in ADAM_BETAS:
    for n in ADAM_NS:
      c = adam_case(n, betas)
      args = (c['p'], c['m'], c['v'], c['grads'], c['lr'], c['b1'], c['b2'], c['eps'])
      ref, lo = adam_ref(*args), adam_ref(*args, dtype=np.float32)
      sc = adam_scales(c, ref)
      for t in range(ADAM_STEPS):
        for k, e in adam_errors(lo[t], ref[t], sc[t]).items():
          worst[betas][k][t] = max(worst[betas][k][t], e)
  return worst


# ================================================================================================ TD epilogue
TD_SHAPES = ((1, 1), (3, 5), (5, 255), (5, 256), (5, 257), (33, 625), (32, 2401), (32, 9409))
# (use_double, huber_delta, weights, reward_scale): every switch with both values
TD_SWITCHES = ((True, 1.0, True, 0.0), (False, 0.25, False, 0.75), (True, None, False, 0.75), (False, None, True, 0.0))
TD_CASES = tuple((mb, A) + s for (mb, A) in ((3, 5), (32, 2401)) for s in TD_SWITCHES) + \
    tuple((mb, A) + TD_SWITCHES[i % 4] for i, (mb, A) in enumerate(((1, 1), (5, 255), (5, 256), (5, 257), (33, 625), (32, 9409)))) + \
    ((1, 1) + TD_SWITCHES[1], (32, 9409) + TD_SWITCHES[0], (33, 625) + TD_SWITCHES[2], (5, 257) + TD_SWITCHES[0])
TD_GAMMA = 0.966667
TD_PRIO_EPS = 1e-3


def td_case(mb, A, double, huber, use_w, reward_scale, seed=0):
  """Inputs of one TD epilogue call, with the designed samples where the shape has room (`notes` lists what was placed):
    sample 0: a tie at the selecting row's maximum between two threads (indices 1 and 3), not terminal, td == 0
    sample 1: a tie inside one thread (indices 2 and 258), terminal, |td| == delta exactly (rewards on a lattice)
    sample 2: a selecting row of -inf except its last entry, td < -delta
    sample 3: the taken action is the arg-max position."""
  rng = np.random.RandomState(100000 * seed + 31 * mb + A + (1 if double else 0) + (2 if use_w else 0))
  q = (rng.normal(size=(mb, A)) * 2).astype(F)
  qo = rng.normal(size=(mb, A)).astype(F)
  qt = rng.normal(size=(mb, A)).astype(F)
  actions = rng.randint(0, A, size=mb).astype(np.int64)
  rewards = rng.normal(size=mb).astype(F)
  terminal = (rng.rand(mb) < 0.3).astype(np.uint8)
  weights = (rng.rand(mb) + 0.1).astype(F) if use_w else None
  sel = qo if double else qt
  notes = set()
  terminal[0] = 0
  if A >= 4:
    sel[0, 1] = sel[0, 3] = F(9.0); notes.add('tie between threads')
    qt[0, 1], qt[0, 3] = (F(0.75), F(-1.25)) if double else (F(9.0), F(9.0))
    if double:
      qt[0, 0] = F(5.0)                                       # the target net's own arg-max lies elsewhere
  if mb >= 2:
    terminal[1] = 1
    rewards[1] = F(np.round(rewards[1] * 8) / 8)            # y = r [x 0.75]: a multiple of 1 / 32, so that y + delta is exact
    if A > 258:
      sel[1, 2] = sel[1, 258] = F(8.5); notes.add('tie inside a thread')
      if double:
        qt[1, 2], qt[1, 258] = F(0.5), F(-2.0)
  if mb >= 3 and A >= 2:
    keep = qt[2, A - 1] if not double else sel[2, A - 1]
    sel[2, :] = NEG_INF; sel[2, A - 1] = keep; terminal[2] = 0; notes.add('-inf row')
  c = dict(q=q, qo=qo, qt=qt, actions=actions, rewards=rewards, terminal=terminal, weights=weights, gamma=f32s(TD_GAMMA),
           huber=None if huber is None else f32s(huber), reward_scale=f32s(reward_scale), double=bool(double),
           prio_eps=f32s(TD_PRIO_EPS), mb=mb, A=A, notes=notes)
  astar = argmax_ref(sel)
  if mb >= 4:
    actions[3] = astar[3]; notes.add('action == arg-max')
  y32 = td_f32(c)['y']                                      # the target as float32 computes it: q - y is then exact
  delta = F(1.0 if huber is None else huber)
  q[0, actions[0]] = y32[0]; notes.add('td == 0')
  if mb >= 2:
    q[1, actions[1]] = y32[1] + delta; notes.add('|td| == delta')
  if mb >= 3:
    q[2, actions[2]] = y32[2] - F(3) * delta; notes.add('td < -delta')
  return c


def _td(c, T, variant=None):
  mb, A = c['mb'], c['A']
  q, qo, qt = (np.asarray(c[k], T) for k in ('q', 'qo', 'qt'))
  r = np.asarray(c['rewards'], T); term = np.asarray(c['terminal']) != 0
  gamma = T(c['gamma']); rs = T(c['reward_scale']); eps = T(c['prio_eps'])
  rows = np.arange(mb)
  double = c['double']
  sel = (qt if variant == 'arg-max from the wrong network' else qo) if double else qt
  astar = argmax_ref(sel)
  if variant == 'ties to the highest index':
    astar = A - 1 - argmax_ref(np.where(np.isnan(sel), -np.inf, sel)[:, ::-1])
  tq = qt[rows, astar]
  rr = r * rs if c['reward_scale'] != 0.0 else r
  if variant == 'terminal ignored':
    term = np.zeros(mb, bool)
  with np.errstate(invalid='ignore'):
    boot = np.where(term, T(0), gamma * tq)
  y = rr + boot
  if variant == 'reward_scale on the whole target' and c['reward_scale'] != 0.0:
    y = (r + boot) * rs
  act = np.asarray(c['actions'])
  qa = q[rows, act]
  td = qa - y
  ad = np.abs(td)
  if c['huber'] is not None:
    d = T(c['huber'])
    quad = np.minimum(ad, d); lin = ad - quad
    loss = T(0.5) * quad * quad + d * lin
    dq = np.where(td < 0, -quad, quad)
    if variant == 'Huber gradient without its sign':
      dq = quad
  else:
    loss = T(0.5) * ad * ad
    dq = td
  w = np.asarray(c['weights'], T) if c['weights'] is not None else np.ones(mb, T)
  loss = loss * w
  grad = np.zeros((mb, A), T)
  grad[rows, act] = (dq * w) / T(mb)
  sl, st = T(0), T(0)
  for i in range(mb):                                       # the header's means, summed in index order
    sl = sl + loss[i]; st = st + td[i]
  return dict(loss=sl / T(mb), mtd=st / T(mb), td=td, td_abs=ad, logits=np.log(ad + eps), grad_q=grad, astar=astar, y=y,
              loss_j=loss, dq=dq, w=w, qa=qa, rr=rr, boot=boot)


def td_ref(c, variant=None):
  """The header's srl_td_epilogue in float64: loss, mtd, td, td_abs, logits, dense grad_q (and the intermediate terms)."""
  return _td(c, np.float64, variant)


def td_f32(c):
  """The same expressions in float32 on the host, in the header's order: td_abs of the kernel equals this one's exactly."""
  return _td(c, np.float32)


def td_scales(ref):
  """Bounds' scales from the reference.  S_j = |q| + |r| + |gamma tq|: the operands of td.  |d loss_j| <= w (|dq| |d td| + a
  rounding of loss_j); |d grad| <= w / mb (|d td| + a rounding of dq) (dq = td in the quadratic region, a constant outside);
  |d logit| <= |d td| / (|td| + eps) + roundings of the sum and the logarithm, hence the scale 1 + |logit| + S / (|td| + eps);
  the means sum the per-sample terms."""
  S = np.abs(ref['qa']) + np.abs(ref['rr']) + np.abs(ref['boot'])
  w, mb = ref['w'], len(S)
  lj = w * (np.abs(ref['dq']) * S + np.abs(ref['loss_j']) / w)
  return dict(td=S, grad=w / mb * (S + np.abs(ref['dq'])), loss=lj.sum() / mb, mtd=S.sum() / mb,
              logits=1.0 + np.abs(ref['logits']) + S / np.exp(ref['logits']))


# measured (float32 host vs float64 over TD_CASES), in units of 2^-24 scale -> C = 4 x measured
TD_MEASURED = {'td': 1.59, 'grad': 0.774, 'loss': 0.52, 'mtd': 0.426, 'logits': 0.86}     # C = 6.36, 3.1, 2.08, 1.7, 3.44
TD_C = {k: 4.0 * v for k, v in TD_MEASURED.items()}


def td_errors(got, ref):
  """Largest error / (2^-24 scale) per quantity.  `got`: dict(loss, mtd, td_abs, logits, grad_q)."""
  sc = td_scales(ref)
  f = lambda a: np.asarray(a, np.float64)
  act_err = np.abs(f(got['grad_q']) - ref['grad_q']).max(axis=1)
  e = dict(td=float((np.abs(f(got['td_abs']) - ref['td_abs']) / (U * sc['td'])).max()),
           grad=float((act_err / (U * sc['grad'])).max()),
           loss=float(abs(float(got['loss']) - ref['loss']) / (U * sc['loss'])),
           mtd=float(abs(float(got['mtd']) - ref['mtd']) / (U * sc['mtd'])),
           logits=float((np.abs(f(got['logits']) - ref['logits']) / (U * sc['logits'])).max()))
  return e


def measure_td():
  worst = {k: 0.0 for k in TD_MEASURED}
  for case in TD_CASES:
    c = td_case(*case)
    for k, e in td_errors(td_f32(c), td_ref(c)).items():
      worst[k] = max(worst[k], e)
  return worst


# ================================================================================================ Gumbel top-k
TOPK_CHUNK = 2048                               # slots per workgroup of stage 1: 256 threads x 8 slots (i, i + 256, ...)
TOPK_NS = (1, 5, 2047, 2048, 2049, 4097, 40000)
TOPK_KS = (1, 8, 32)


def gumbel_keys(logits, u, alpha, dtype=np.float64):
  T = dtype
  l = np.asarray(logits, T); u = np.asarray(u, T)
  with np.errstate(invalid='ignore', divide='ignore'):
    return np.where(np.isinf(l), T(-np.inf), T(alpha) * l) - np.log(-np.log(u))


def topk_ref(keys, k):
  """keys: float64 [n], or (logits, u, alpha).  (indices int64 [k], keys float64 [k]): descending key, the lower index first
  among equal keys; positions beyond the sampleable slots carry key -inf and index 0."""
  if isinstance(keys, tuple):
    keys = gumbel_keys(*keys)
  keys = np.asarray(keys, np.float64)
  order = np.lexsort((np.arange(len(keys)), -keys))[:k]
  idx = np.zeros(k, np.int64); key = np.full(k, -np.inf)
  ok = keys[order] > -np.inf
  idx[:len(order)] = np.where(ok, order, 0); key[:len(order)] = np.where(ok, keys[order], -np.inf)
  return idx, key


def topk_designed(n, placement):
  """Designed keys: u constant and alpha = 1, logits multiples of 1 / 8 in [-4, 4) with the largest values DUPLICATED at the
  named placement, so the expected order is exact.  Returns (logits, u, alpha)."""
  rng = np.random.RandomState(n + len(placement))
  l = (rng.randint(-32, 32, size=n) / 8.0).astype(F)
  pairs = {'same thread': [(3, 3 + 256), (700, 700 + 512)], 'two threads': [(5, 6), (300, 900)],
           'two chunks': [(0, TOPK_CHUNK), (100, n - 2)], 'ragged chunk': [(n - 2, n - 1), (n - 40, n - 3)]}[placement]
  for j, (a, b) in enumerate(pairs):
    assert 0 <= a < b < n
    l[a] = l[b] = F(8.0 - j)                              # above the lattice: both pairs lead the order, equal inside a pair
  return l, np.full(n, 0.5, F), 1.0


TOPK_DESIGNED = (('same thread', 2049), ('same thread', 40000), ('two threads', 2047), ('two threads', 2048),
                 ('two chunks', 2049), ('two chunks', 4097), ('two chunks', 40000), ('ragged chunk', 2047),
                 ('ragged chunk', 4200), ('ragged chunk', 40000))
# (name, n, k, sampleable slots): where the finite logits sit
TOPK_PLACEMENTS = (('first chunk', 40000, 32, tuple(range(3, 2048, 41))), ('middle chunk', 40000, 32, tuple(range(20480, 22528, 37))),
                   ('last chunk', 40000, 32, tuple(range(38912, 40000, 23))),
                   ('3 per chunk', 40000, 32, tuple(c * 2048 + o for c in range(20) for o in (1, 700 + c, 1999 - 17 * c) if c * 2048 + o < 40000)),
                   ('3 per chunk, 17 chunks', 32769 + 2048, 32, tuple(c * 2048 + o for c in range(17) for o in (0, 257, 2047))),
                   ('fewer than k', 4097, 8, (5, 2048, 4096)), ('fewer than k', 40000, 32, tuple(range(11, 40000, 3000))),
                   ('fewer than k', 5, 8, (1, 4)), ('none', 2049, 8, ()))
TOPK_RANDOM = tuple((n, k) for n in TOPK_NS for k in TOPK_KS)
TOPK_ALPHA = 0.6


def topk_random(n, k, seed=0):
  rng = np.random.RandomState(17 * n + k + seed)
  l = (rng.normal(size=n) * 2).astype(F)
  if n > 1:
    l[rng.rand(n) < 0.3] = NEG_INF
  u = rng.uniform(1e-6, 1.0 - 1e-6, size=n).astype(F)
  return l, u, f32s(TOPK_ALPHA)


def topk_placement(n, slots, seed=0):
  rng = np.random.RandomState(n + len(slots) + seed)
  l = np.full(n, NEG_INF, F)
  l[list(slots)] = (rng.normal(size=len(slots)) * 2).astype(F)
  return l, rng.uniform(1e-6, 1.0 - 1e-6, size=n).astype(F), f32s(TOPK_ALPHA)


def topk_key_scale(logits, u, alpha, idx):
  """1 + |alpha logit| + |Gumbel term| at the returned slots: the key is a product, two logarithms and a difference (the inner
  logarithm's rounding enters the outer one's argument relatively: at most a unit, the 1)."""
  l = np.asarray(logits, np.float64)[idx]; uu = np.asarray(u, np.float64)[idx]
  with np.errstate(invalid='ignore'):
    return 1.0 + np.where(np.isinf(l), 0.0, np.abs(alpha * l)) + np.abs(np.log(-np.log(uu)))


# measured: float32 host keys against float64 over TOPK_RANDOM, all slots, in units of 2^-24 scale -> C = 4 x measured
TOPK_MEASURED = 2.21           # C = 8.84
TOPK_C = 4.0 * TOPK_MEASURED


def measure_topk():
  worst = 0.0
  for n, k in TOPK_RANDOM:
    l, u, a = topk_random(n, k)
    fin = np.flatnonzero(np.isfinite(l))
    if len(fin):
      with np.errstate(invalid='ignore'):
        d = np.abs(gumbel_keys(l, u, a, np.float32).astype(np.float64) - gumbel_keys(l, u, a))[fin]
      e = d / (U * topk_key_scale(l, u, a, fin))
      worst = max(worst, float(e.max()))
  return worst


def topk_decided(logits, u, alpha, k):
  """(reference indices, reference keys, mask [k]): mask marks the returned positions whose float64 key is further than twice
  the key tolerance from both neighbours in the order (the k + 1-th included): there the float32 order cannot differ."""
  keys = gumbel_keys(logits, u, alpha)
  idx, key = topk_ref(keys, k + 1)
  tol = np.where(np.isfinite(key), TOPK_C * U * topk_key_scale(logits, u, alpha, idx), 0.0)
  with np.errstate(invalid='ignore'):
    gap = key[:-1] - key[1:]                              # nan between two -inf entries: undecided is right (both are flags)
    sep = gap > 2 * (tol[:-1] + tol[1:])
  sep = np.where(np.isnan(gap), True, sep)
  mask = np.concatenate([[True], sep[:-1]]) & sep
  return idx[:k], key[:k], mask[:k]


# ================================================================================================ replay scatter / gather
REPLAY_ROW_BYTES = ((16, 16), (48, 16), (8192, 256), (32768, 1024), (65536, 32))
REPLAY_BS = (1, 7)
REPLAY_PART_LENS = (1, 9)
REPLAY_N_STEPS = (1, 3)
SCATTER_GRID_CAP, GATHER_GRID_CAP = 16, 32      # x-grid caps of the two launches: 256 lanes of 16 bytes per block


def replay_memory(B, part_len, bytes0, bytes1, seed=0):
  """A memory of B partitions of part_len rows, every tensor filled with a recognisable pattern (not zeros): the `sentinel`
  the scatter must leave alone.  Logits: a mix of finite values and -inf."""
  rng = np.random.RandomState(B * 131 + part_len * 7 + bytes0 % 1000 + seed)
  N = B * part_len
  lg = rng.normal(size=N).astype(F); lg[rng.rand(N) < 0.25] = NEG_INF
  return dict(m0=rng.randint(0, 256, (N, bytes0)).astype(np.uint8), m1=rng.randint(0, 256, (N, bytes1)).astype(np.uint8),
              reward=rng.normal(size=N).astype(F), terminal=(rng.rand(N) < 0.5).astype(np.uint8),
              action=rng.randint(0, 9409, N).astype(np.int64), logits=lg)


def replay_transitions(B, bytes0, bytes1, seed=0):
  rng = np.random.RandomState(B + bytes1 + seed + 5)
  return dict(s0=rng.randint(0, 256, (B, bytes0)).astype(np.uint8), s1=rng.randint(0, 256, (B, bytes1)).astype(np.uint8),
              reward=rng.normal(size=B).astype(F), terminal=(rng.rand(B) < 0.5).astype(np.uint8),
              action=rng.randint(0, 9409, B).astype(np.int64))


def scatter_ref(mem, tr, slot, part_len):
  """The header's srl_replay_scatter on a copy of the whole memory: transition b to row b part_len + slot, its logit -inf."""
  out = {k: v.copy() for k, v in mem.items()}
  for b in range(tr['s0'].shape[0]):
    row = b * part_len + slot
    out['m0'][row] = tr['s0'][b]; out['m1'][row] = tr['s1'][b]
    out['reward'][row] = tr['reward'][b]; out['terminal'][row] = tr['terminal'][b]; out['action'][row] = tr['action'][b]
    out['logits'][row] = NEG_INF
  return out


def next_rows(idx, part_len, n_steps, literal):
  idx = np.asarray(idx, np.int64)
  if literal:
    return (idx + n_steps) % part_len + idx // part_len                      # the formula as the reference wrote it
  return (idx % part_len + n_steps) % part_len + (idx // part_len) * part_len   # n_steps on inside the partition


def gather_ref(mem, idx, part_len, n_steps, literal, alpha=None, beta=None, min_logit=None):
  """The header's srl_replay_gather: rows idx and their next rows of both state tensors, action of the row, reward and
  terminal flag of the next row, the next-row indices, and the float64 importance weight (and its exponent)."""
  idx = np.asarray(idx, np.int64)
  nxt = next_rows(idx, part_len, n_steps, literal)
  out = dict(s0=mem['m0'][idx], s1=mem['m1'][idx], n0=mem['m0'][nxt], n1=mem['m1'][nxt], action=mem['action'][idx],
             reward=mem['reward'][nxt], terminal=mem['terminal'][nxt], next=nxt)
  if alpha is not None:
    arg = float(beta) * float(alpha) * (float(min_logit) - mem['logits'][idx].astype(np.float64))
    out['weight_arg'] = arg; out['weight'] = np.exp(arg)
  return out


def gather_indices(B, part_len):
  """A partition's last slot (the next row wraps), the last partition, the first row, a repeated index."""
  N = B * part_len
  return np.array([part_len - 1, N - 1, 0, (B - 1) * part_len, part_len // 2, 0, N - 1], np.int64)


GATHER_ALPHA, GATHER_BETA = 0.6, 0.7
# measured: float32 host weight exp(beta alpha (min - logit)) against float64, relative, in units of 2^-24 (1 + |argument|)
WEIGHT_MEASURED = 1.52         # C = 6.08
WEIGHT_C = 4.0 * WEIGHT_MEASURED


def weight_f32(mem, idx, alpha, beta, min_logit):
  return np.exp(F(beta) * F(alpha) * (F(min_logit) - mem['logits'][np.asarray(idx)]))


def finite_rows(mem):
  return np.flatnonzero(np.isfinite(mem['logits']))


def measure_weight():
  worst = 0.0
  for B in REPLAY_BS:
    for L in REPLAY_PART_LENS:
      mem = replay_memory(B, L, 16, 16)
      idx = finite_rows(mem)
      if not len(idx):
        continue
      mn = float(mem['logits'][idx].min())
      ref = gather_ref(mem, idx, L, 1, False, f32s(GATHER_ALPHA), f32s(GATHER_BETA), mn)
      got = weight_f32(mem, idx, f32s(GATHER_ALPHA), f32s(GATHER_BETA), mn).astype(np.float64)
      worst = max(worst, float((np.abs(got / ref['weight'] - 1) / (U * (1 + np.abs(ref['weight_arg'])))).max()))
  return worst


# ================================================================================================ logit extrema
EXTREMA_BLOCK, EXTREMA_MAX_BLOCKS, EXTREMA_PER_BLOCK = 256, 256, 1024
EXTREMA_NS = (1, 5, 255, 256, 257, 1024, 65536, 262144, 262145, 300001)


def extrema_ref(logits):
  """(max, its lowest index, min FINITE logit, its lowest index); (+inf, 0) for the minimum when no logit is finite."""
  x = np.asarray(logits, np.float64)
  imx = int(np.argmax(x))
  fin = np.isfinite(x)
  if not fin.any():
    return float(x[imx]), imx, np.inf, 0
  imn = int(np.argmin(np.where(fin, x, np.inf)))
  return float(x[imx]), imx, float(x[imn]), imn


def extrema_cases(n, seed=0):
  """[(name, logits float32 [n])]"""
  rng = np.random.RandomState(n + seed)
  base = rng.normal(size=n).astype(F)
  if n > 2:
    base[rng.rand(n) < 0.3] = NEG_INF
  out = []
  x = base.copy()
  if n >= 4:
    x[n // 2] = x[n - 1] = F(7.5); x[1] = x[n // 3] = F(-9.25)
  out.append(('ties and -inf', x))
  out.append(('all -inf', np.full(n, NEG_INF, F)))
  x = base.copy(); x[n // 2] = np.inf
  if n >= 2:
    x[0] = F(-3.0)                                              # a finite entry: the minimum
  out.append(('+inf', x))
  if n > 2 * EXTREMA_BLOCK:                                      # two maxima that two different workgroups see first
    x = base.copy(); a = EXTREMA_BLOCK + 3; b = n - 2
    x[a] = x[b] = F(6.0); x[5] = F(-8.0); x[n - 1] = F(-8.0)
    out.append(('tie across blocks', x))
  return out
