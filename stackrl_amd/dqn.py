"""DQN agent of the rollout/update path: `DQN` (stackrl/agents/dqn.py:19-486) on PyTorch-ROCm.

Same surface as the reference: `collect` (:391-395), `observe` (:387-389), `train` (:397-486), `policy` (:330-375),
`acknowledge_reset` (:381-385), `iterations`, `epsilon`, `exploration`, `replay_memory_size`.  Epsilon-greedy or
Boltzmann (Gumbel-max) exploration, Huber TD loss, Double-DQN, n-step returns, prioritised replay with
importance-sampling weights, hard target sync every `target_update_period` iterations.

Multi-GPU (absent in the reference): one process per GPU, env shard + replay shard per rank, and ONE collective
per update — an all-reduce (RCCL over xGMI) of the flat gradient bucket (~2.13 M fp32 = 8.5 MB), averaged.
All gradients are views of one contiguous buffer, so the collective needs no packing copies.
"""
import collections
import math

import torch
import torch.distributed as dist

from stackrl_amd.memory import ReplayMemory


# Stream captures run in thread-local error mode: with a process group alive (RCCL's watchdog thread polls its events)
# another thread's HIP calls must not invalidate a capture in progress on this one
CAPTURE_MODE = 'thread_local'


class PolynomialDecay(object):
  """keras.optimizers.schedules.PolynomialDecay (config.gin:73-81), cycle=False."""

  def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0):
    self.initial, self.steps, self.end, self.power = float(initial_learning_rate), int(decay_steps), float(end_learning_rate), float(power)

  def __call__(self, step):
    s = min(int(step), self.steps)
    return (self.initial - self.end) * (1 - s / self.steps) ** self.power + self.end


EXPLORATION_MODES = ['epsilon-greedy', 'boltzmann']     # dqn.py:23-28


def philox4x32_10(counter, key):
  """Philox4x32-10: counter int64 [..., 4], key int64 [..., 2] (32-bit words in int64 elements, broadcast against each
  other) -> int64 [..., 4].  The product of two 32-bit words wraps in int64; its low and high words are read by mask and
  shift.  Pure torch, either device."""
  c0, c1, c2, c3 = (counter[..., i] & 0xffffffff for i in range(4))
  k0, k1 = key[..., 0] & 0xffffffff, key[..., 1] & 0xffffffff
  for _ in range(10):
    p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
    c0, c1, c2, c3 = ((p1 >> 32) & 0xffffffff) ^ c1 ^ k0, p1 & 0xffffffff, ((p0 >> 32) & 0xffffffff) ^ c3 ^ k1, p0 & 0xffffffff
    k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
  return torch.stack((c0, c1, c2, c3), dim=-1)


def boltzmann_uniform(x, dtype=torch.float32):
  """The uniform number of a 32-bit Philox word: ((x >> 9) + 0.5) * 2^-23, exact in float32, within [2^-24, 1 - 2^-24]."""
  return ((x >> 9).to(dtype) + 0.5) * 2.0 ** -23


def boltzmann_noise(keys, A, dtype=torch.float32):
  """The Gumbel noise z [B, A] of the Boltzmann head for the stream keys [B, 2] (int64; one per sample), by the definition
  in include/stackrl_explore.h, which the kernel `k_boltzmann_head` computes in registers: action a of sample b takes
  word a % 4 of Philox4x32-10(counter (a // 4, 0, 0, 0), key keys[b]).  Pure torch, either device."""
  quads = (int(A) + 3) // 4
  counter = torch.zeros((1, quads, 4), dtype=torch.int64, device=keys.device)
  counter[0, :, 0] = torch.arange(quads, dtype=torch.int64, device=keys.device)
  x = philox4x32_10(counter, keys[:, None, :]).reshape(keys.shape[0], 4 * quads)[:, :int(A)]
  return -torch.log(-torch.log(boltzmann_uniform(x, dtype)))


def greedy_head_reference(adv, v, n_valid=None):
  """The greedy head by the definition in include/stackrl_greedy.h, which the kernel `k_greedy_head` computes in one pass per
  env: adv [B, A] or [B, G, A] float32 (G rows per env, the first `n_valid` valid; None = all), v [B] float32 or None (not
  dueling: q = adv) -> (actions [B] int64, the flat index r * A + p with ties to the lowest; stats [B, 4] float64 {max q, min q,
  sum q, sum q^2} over the valid rows; q float32 in the shape of adv, rows beyond n_valid -inf).  Pure torch, either device."""
  flat2 = adv.dim() == 2
  a = (adv[:, None] if flat2 else adv).float()
  B, G, A = a.shape
  n_valid = G if n_valid is None else int(n_valid)
  if not 1 <= n_valid <= G:
    raise ValueError('n_valid must be in 1..{}, got {}'.format(G, n_valid))
  a = a[:, :n_valid]
  if v is None:
    qv = a
  else:
    m = (a.double().sum(dim=-1, keepdim=True) / A).float()           # float64 sum, one rounding to float32
    qv = (a - m) + v.reshape(B, 1, 1).float()                        # models.py:188-192, in this order
  flat = qv.reshape(B, n_valid * A)
  nan = torch.isnan(flat)
  top = torch.where(nan, torch.full_like(flat, -float('inf')), flat)  # a NaN never wins; nothing but NaN / -inf: index 0
  actions = torch.argmax(top, dim=-1)
  d = flat.double()
  stats = torch.stack((top.amax(dim=-1).double(), torch.where(nan, torch.full_like(flat, float('inf')), flat).amin(dim=-1).double(),
                       d.sum(dim=-1), (d * d).sum(dim=-1)), dim=-1)
  q = torch.full((B, G, A), -float('inf'), dtype=torch.float32, device=adv.device)
  q[:, :n_valid] = qv
  return actions, stats, (q[:, 0] if flat2 else q)


class KerasAdam(object):
  """`keras.optimizers.Adam` as the reference applies it (dqn.py:473; config.gin:90-93) over ONE flat fp32 bucket:
  m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); p -= lr_t m / (sqrt(v) + eps), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
  (epsilon outside the bias correction, unlike torch.optim.Adam).  The parameters are re-pointed to views of the
  bucket, so a step is one launch of `srl_adam_step` (csrc/learner.hip) on a HIP device — capturable, the step counter
  and its powers live in device memory — and the same formula in torch on the CPU (host-logic tests)."""

  ALIGN = 64   # every parameter starts on a 256-byte boundary of the bucket (library kernels load weights in vectors)

  @classmethod
  def layout(cls, params):
    """Offsets of the parameters in a flat bucket and the bucket's length (elements)."""
    offs, o = [], 0
    for p in params:
      offs.append(o)
      o += (p.numel() + cls.ALIGN - 1) // cls.ALIGN * cls.ALIGN
    return offs, o

  def __init__(self, params, lr=0.001, betas=(0.9, 0.999), eps=1e-7):
    self.params = list(params)
    dev = self.params[0].device
    self.lr, (self.b1, self.b2), self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
    offs, n = self.layout(self.params)
    self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
    with torch.no_grad():
      for p, o in zip(self.params, offs):
        self.flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
        p.data = self.flat[o:o + p.numel()].view_as(p)
    self.m = torch.zeros_like(self.flat)
    self.v = torch.zeros_like(self.flat)
    self.state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32, device=dev)   # t, b1^t, b2^t, lr_t

  @torch.no_grad()
  def step(self, flat_grad):
    if self.flat.is_cuda:
      from stackrl_amd import qops
      qops.adam_step(self.flat, flat_grad, self.m, self.v, self.state, self.lr, self.b1, self.b2, self.eps)
      return
    st = self.state
    st[0] += 1.0; st[1] *= self.b1; st[2] *= self.b2
    st[3] = self.lr * torch.sqrt(1.0 - st[2]) / (1.0 - st[1])
    self.m += (flat_grad - self.m) * (1.0 - self.b1)
    self.v += (flat_grad * flat_grad - self.v) * (1.0 - self.b2)
    self.flat -= (st[3] * self.m) / (torch.sqrt(self.v) + self.eps)

  def state_dict(self):
    return {'m': self.m.clone(), 'v': self.v.clone(), 'state': self.state.clone()}

  def load_state_dict(self, d):
    self.m.copy_(d['m']); self.v.copy_(d['v']); self.state.copy_(d['state'])


# stages: run in this order; stream: 'main' (the caller's current stream) or 'update' (the agent's own); graph: replayed from
# one hipGraph; draws: that graph samples the replay memory, so the sampling generator is registered with it
Segment = collections.namedtuple('Segment', 'stages stream graph draws')


def update_plan(prefetch, world, early, graphs):
  """Where the stages of one minibatch update run: the list of its `Segment`s in execution order.  The stages are grad (the
  minibatch at the head of the FIFO, or a fresh draw without prefetch; target evaluations, forward, loss, backward), fifo
  (shift the slots, draw into the tail; only with prefetch), reduce (all-reduce of the gradient bucket; only with more than
  one rank), apply (average, optimiser step, priorities), always in this order.  `reduce` is a segment of its own and never
  part of a graph: the collective stays an ordinary stream-ordered call of whatever backend the process group has.  With
  `early` (needs prefetch >= 1) so is `grad`, on the update stream, where `train_begin` starts it beside the collect step."""
  early = bool(early) and prefetch >= 1
  groups = [['grad'], []] if early else [['grad']]
  if prefetch:
    groups[-1].append('fifo')
  if world > 1:
    groups += [['reduce'], []]
  groups[-1].append('apply')
  draw = 'fifo' if prefetch else 'grad'
  return [Segment(tuple(g), 'update' if early and i == 0 else 'main', bool(graphs) and g != ['reduce'],
                  bool(graphs) and draw in g) for i, g in enumerate(groups)]


def _clone_slot(slot):
  return tuple(None if t is None else t.clone() for t in slot)


def _copy_slot(dst, src):
  for d, s in zip(dst, src):
    if d is not None:
      d.copy_(s)


class MinibatchFifo(object):
  """`dataset.prefetch(prefetch)` (dqn.py:247-252; config.gin:104 sets 3), restated deterministically.  The reference's
  background thread keeps `prefetch` minibatches sampled AHEAD of the update that consumes them, so a minibatch was drawn —
  with the priorities, the importance-weight schedule and the transitions of that moment — about `prefetch` updates before
  it is used.  Here: `length` slots, filled by as many draws before the first update; every update takes a copy of the
  oldest, and a new one is drawn in its place before the update's own priorities are written (the producer thread refills as
  soon as a slot is free).  The slots live at fixed addresses (shift copies), so the whole thing replays from a hipGraph."""

  def __init__(self, length, draw, device):
    self.length, self._draw, self.device, self.slots = int(length), draw, device, None

  def fill(self):
    if self.slots is None:
      self.slots = [_clone_slot(self._draw()) for _ in range(self.length)]

  def head(self):
    return _clone_slot(self.slots[0])

  def advance(self):
    for dst, src in zip(self.slots, self.slots[1:]):
      _copy_slot(dst, src)
    _copy_slot(self.slots[-1], self._draw())

  def state(self):
    return [_clone_slot(slot) for slot in self.slots]

  def load(self, saved, captured):
    """After the replay memory was restored.  saved: the `state()` of the saved run, or None; captured: a captured update
    reads the slots at their addresses, so they stay."""
    if saved is not None and len(saved) == self.length:
      if self.slots is None:
        self.slots = [tuple(None if t is None else torch.empty_like(t, device=self.device) for t in slot) for slot in saved]
      for dst, src in zip(self.slots, saved):
        _copy_slot(dst, src)
    elif self.slots is not None and not captured:
      self.slots = None                      # minibatches drawn from the memory that was just replaced
    elif self.slots is not None:
      for slot in self.slots:
        _copy_slot(slot, self._draw())


class DQN(object):
  def __init__(self, q_net, optimizer=None, learning_rate=None, huber_delta=1., minibatch_size=32,
               replay_memory_size=100000, prefetch=None, target_update_period=10000, reward_scale=None,
               discount_factor=.99, collect_batch_size=None, exploration_mode=None, exploration=None,
               prioritization=None, priority_bias_compensation=None, double=False, n_step=None, seed=None,
               device=None, process_group=None, policy_op=None, reference_next_index=True,
               adam_betas=(0.9, 0.999), xcorr=None, graphs=False, hand_convs=None, early_gradient=False):
    if not isinstance(q_net, torch.nn.Module):
      raise TypeError('Invalid type {} for argument q_net. Must be a torch Module.'.format(type(q_net)))   # dqn.py:122-125
    self.device = torch.device(device) if device is not None else next(q_net.parameters()).device
    self._q_net = q_net.to(self.device)
    # xcorr: how `layers.correlation` (layers.py:21-38) is evaluated and differentiated in the update.  None keeps the
    # net's own (library grouped convolution, fp32); 'bf16x3' / 'bf16' use the MFMA kernels of csrc/xcorr_mfma.hip
    # (hi/lo-split fp32-class accuracy / operands rounded to bf16) on a HIP device.
    if xcorr is not None:
      if xcorr not in ('bf16x3', 'bf16'):
        raise ValueError("Invalid value {} for argument xcorr. Must be None, 'bf16x3' or 'bf16'.".format(xcorr))
      if self.device.type == 'cuda' and hasattr(self._q_net, 'correlation'):
        from stackrl_amd import qops
        self._q_net.correlation = qops.correlation(qops.BF16X3 if xcorr == 'bf16x3' else qops.BF16)
    # on a HIP device the bias add + ReLU of every convolution (forward, backward and the bias-gradient reduction) are
    # the fused passes of csrc/epilogue.hip
    if self.device.type == 'cuda' and hasattr(self._q_net, 'set_fused_epilogues'):
      self._q_net.set_fused_epilogues(True)
    self._pg = process_group
    self._world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
    if self._world > 1:
      # replicas must start from the same weights whatever seed each rank built its net with: rank 0's are broadcast
      # (the gradient all-reduce keeps them equal from then on)
      src = dist.get_global_rank(process_group, 0) if process_group is not None else 0
      with torch.no_grad():
        for t in list(self._q_net.parameters()) + list(self._q_net.buffers()):
          dist.broadcast(t, src=src, group=process_group)
    import copy
    self._target_q_net = copy.deepcopy(self._q_net)                 # clone + set_weights, dqn.py:116-117
    for p in self._target_q_net.parameters():
      p.requires_grad_(False)
    # one flat gradient bucket; every p.grad is a view into it
    params = [p for p in self._q_net.parameters() if p.requires_grad]
    offs, n = KerasAdam.layout(params)        # the same (256-byte aligned) layout as the optimiser's parameter bucket
    self._flat_grad = torch.zeros(n, dtype=torch.float32, device=self.device)
    for p, o in zip(params, offs):
      p.grad = self._flat_grad[o:o + p.numel()].view_as(p)
    self._params = params
    if optimizer is None:                                            # dqn.py:127-130: Adam with Keras' defaults
      optimizer = KerasAdam(params, lr=learning_rate or 0.00025, betas=adam_betas, eps=1e-7)
    elif callable(optimizer) and not isinstance(optimizer, torch.optim.Optimizer):
      optimizer = optimizer(params, lr=learning_rate or 0.00025)
    elif not isinstance(optimizer, (torch.optim.Optimizer, KerasAdam)):
      raise TypeError('Invalid type {} for argument optimizer.'.format(type(optimizer)))
    self._optimizer = optimizer
    self._iterations = 0
    # exploration (dqn.py:140-187)
    if exploration_mode is None:
      self._exploration_mode = EXPLORATION_MODES[0]
    elif isinstance(exploration_mode, int):
      self._exploration_mode = EXPLORATION_MODES[exploration_mode]
    elif isinstance(exploration_mode, str):
      if exploration_mode.lower() not in EXPLORATION_MODES:
        raise ValueError('Invalid value {} for argument exploration_mode. Must be in {}.'.format(exploration_mode, EXPLORATION_MODES))
      self._exploration_mode = exploration_mode.lower()
    else:
      raise TypeError('Invalid type {} for argument exploration_mode. Must be int or str.'.format(type(exploration_mode)))
    if exploration is None:
      exploration = 0.1 if self._exploration_mode == 'epsilon-greedy' else 1.
    dummy = exploration(0) if callable(exploration) else exploration
    if self._exploration_mode == 'epsilon-greedy' and (dummy < 0 or dummy > 1):
      raise ValueError('Invalid value {} for argument exploration. Must be in [0,1].'.format(exploration))
    if self._exploration_mode == 'boltzmann' and dummy <= 0:
      raise ValueError('Invalid value {} for argument exploration. Must be greater than 0.'.format(exploration))
    self._exploration = exploration
    self._huber = huber_delta is not None                            # dqn.py:189-192
    self._huber_delta = float(huber_delta) if self._huber else None
    self._target_update_period = target_update_period or 10000
    n_step = n_step or 1                                             # dqn.py:195-211
    self._n_step = n_step > 1
    if self._n_step:
      self._gamma_r = torch.tensor([discount_factor ** i for i in range(n_step)], dtype=torch.float32, device=self.device)
      self._gamma = float(discount_factor ** n_step)
    else:
      self._gamma = float(discount_factor)
    self._reward_scale = float(reward_scale) if reward_scale else None
    self._minibatch_size = int(minibatch_size)
    collect_batch_size = collect_batch_size or 1
    self._n_actions = int(q_net.n_actions)
    prioritization = prioritization or 0.                            # dqn.py:229-235
    self._prioritized = prioritization != 0.
    self._bias_compensation = False
    if self._prioritized:
      if priority_bias_compensation is None:
        priority_bias_compensation = 1.
      self._bias_compensation = callable(priority_bias_compensation) or priority_bias_compensation != 0.
    (H, W), (h, w) = getattr(q_net, 'in_hw', ((128, 128), (32, 32)))
    state_spec = (((collect_batch_size, H, W, 2), torch.uint8), ((collect_batch_size, h, w, 1), torch.uint8))
    self._replay_memory = ReplayMemory(state_spec, replay_memory_size, alpha=prioritization,
                                       beta=priority_bias_compensation, iters_counter=lambda: self._iterations,
                                       n_steps=n_step, seed=seed, device=self.device,
                                       reference_next_index=reference_next_index)
    self._double = double
    # prefetch: how many minibatches are sampled ahead of the update that uses them (dqn.py:247-252; None / 0 = none)
    self._prefetch = int(prefetch or 0)
    self._fifo = MinibatchFifo(self._prefetch, self._draw, self.device) if self._prefetch else None
    self._last_sample_indexes = None
    self._gen = torch.Generator(device=self.device)
    if seed is not None:
      self._gen.manual_seed(int(seed) + 1)
    self._policy_op = policy_op     # optional fused rollout head (stackrl_amd.qops.FusedPolicy)
    self.policy_timer = None        # optional object with start() / stop() called around every policy evaluation (bench.py)
    # graphs: the update — prioritised sampling, target evaluation, forward, backward, Adam, priority update: hundreds of
    # launches of mostly microsecond kernels — replayed from hipGraphs, one per graphed segment of `update_plan` (HIP device
    # only).  Everything they read or write lives at fixed addresses (replay tensors, trackers, FIFO slots, flat gradient and
    # parameter buckets, Adam state, schedule scalars) and the nets' parameters are updated in place, so target syncs and
    # checkpoints need no re-capture.  The first `_GRAPH_WARMUP` updates are eager and serial.
    self._graphs = bool(graphs) and self.device.type == 'cuda'
    # early_gradient: `train_begin()` starts the gradient half of the next update — target evaluation, forward, loss,
    # backward, on the minibatch at the head of the prefetch FIFO, which was drawn `prefetch` updates ago and does not depend
    # on the collect step of this iteration — on a stream of its own, beside the collect step; `train()` then completes the
    # update (new minibatch into the FIFO, all-reduce, optimiser step, priorities).  Same operations on the same operands in
    # the same order per tensor as the serial update: identical results (tests/test_learner_gpu.py).  Needs prefetch >= 1.
    self._early = bool(early_gradient) and self.device.type == 'cuda' and self._prefetch >= 1
    self._upd_stream = torch.cuda.Stream(device=self.device) if self._early else None
    self._plan = update_plan(self._prefetch, self._world, self._early, self._graphs)
    self._warmup_plan = update_plan(self._prefetch, self._world, False, False)
    self._warmup = self._GRAPH_WARMUP if self._graphs else 0
    self._updates = 0                       # updates run by this object (a restored `iterations` is not that)
    self._captured = {}                     # index of a graphed segment of `_plan` -> its hipGraph
    self._running = None                    # the plan of an update whose first segment has run and the others not yet
    self._out = None                        # what `grad` returned
    # the loss and its gradient as one hand-written kernel (csrc/learner.hip) on a HIP device
    self._fused = self.device.type == 'cuda'
    self._ws = {}
    # hand_convs: every convolution of the update (forward with saved activations, data gradient, weight gradient) on the
    # kernels of csrc/train_conv.hip instead of the library's (stackrl_amd/qtrain.py; None = on a HIP device whenever the
    # net and the optimiser allow it: the config.gin network over the flat Keras-Adam bucket)
    self._hand = self._hand_t = None
    self._hand_cover_checked = False
    if hand_convs is None:
      hand_convs = self._fused and isinstance(self._optimizer, KerasAdam) and self._hand_supported()
    if hand_convs:
      from stackrl_amd import qtrain
      self._hand = qtrain.HandNet(self._q_net, flat=self._optimizer.flat)
      self._hand_t = qtrain.HandNet(self._target_q_net)
      self._hand_t.refresh()

  def _hand_supported(self):
    """`qtrain.HandNet` covers the config.gin network: a `DeepQSiamFCN` with the dueling head on average-pooled features,
    two position layers, and the observation sizes the cross-correlation kernels are built for."""
    from stackrl_amd import nets, qops
    n = self._q_net
    if not isinstance(n, nets.DeepQSiamFCN) or not n.dueling or not n.dueling_avg_pool or len(n.pos) != 5:
      return False
    (H, W), (h, w) = n.in_hw
    chans = [m.out_channels for m in n.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)) and m.out_channels > 1]
    return H == W and h == w and (H, h) in qops.MFMA_SHAPES and all(c % 16 == 0 and c <= 256 for c in chans)

  def __call__(self, state, reward, terminal, action=None):
    return self.collect(state, reward, terminal) if action is None else self.observe(state, reward, terminal, action)

  # ------------------------------------------------------------------ properties (dqn.py:307-328)
  @property
  def iterations(self):
    return self._iterations

  @property
  def replay_memory_size(self):
    return self._replay_memory.max_length

  @property
  def exploration(self):
    return float(self._exploration(self._iterations)) if callable(self._exploration) else float(self._exploration)

  @property
  def epsilon(self):
    if self._exploration_mode == 'epsilon-greedy':
      return self.exploration
    return math.exp(-1 / self.exploration)

  @property
  def q_net(self):
    return self._q_net

  # ------------------------------------------------------------------ policy (dqn.py:330-375)
  def policy_draws(self, batch_size):
    """The random numbers one exploring `policy` call over `batch_size` samples consumes, drawn as that call draws them.
    A policy evaluated group by group (`PipelinedVecStackEnv.collect_step`) hands each group its slice (`draws=`) and
    takes the actions one call over the whole batch would take.  Every element of the tuple is indexed by sample:
    epsilon-greedy draws (u, random action), Boltzmann one Philox stream key per sample, (keys [B, 2],) (`boltzmann_noise`)."""
    dev = next(self._q_net.parameters()).device
    if self._exploration_mode == 'boltzmann':
      return (torch.randint(0, 2 ** 32, (batch_size, 2), dtype=torch.int64, generator=self._gen, device=dev),)
    u = torch.rand(batch_size, generator=self._gen, device=dev)
    return u, torch.randint(self._n_actions, (batch_size,), generator=self._gen, device=dev)

  @torch.no_grad()
  def policy(self, inputs, exploration=False, values=False, draws=None):
    timer = self.policy_timer
    if timer is not None:
      timer.start()
    try:
      return self._policy(inputs, exploration, values, draws)
    finally:
      if timer is not None:
        timer.stop()

  def _policy(self, inputs, exploration, values, draws):
    if self._policy_op is not None and exploration and not values:
      # epsilon or, in Boltzmann mode, the temperature
      return self._policy_op(self._q_net, inputs, self.exploration, self._gen, draws=draws, mode=self._exploration_mode)
    with torch.no_grad():
      q = self._q_net(inputs)
    greedy = torch.argmax(q, dim=-1)                 # ties -> lowest index
    if exploration:
      e = self.exploration
      if self._exploration_mode == 'epsilon-greedy':
        u, rnd = draws if draws is not None else self.policy_draws(q.shape[0])
        actions = torch.where(u > e, greedy, rnd)
      elif draws is not None:                        # per-sample streams: any partition of the batch takes the same actions
        actions = torch.argmax(q / e + boltzmann_noise(draws[0], q.shape[-1], q.dtype), dim=-1)
      else:
        z = -torch.log(-torch.log(torch.rand(q.shape, generator=self._gen, device=q.device)))
        actions = torch.argmax(q / e + z, dim=-1)
    else:
      actions = greedy
    return (actions, q) if values else actions

  @torch.no_grad()
  def greedy(self, inputs, stats=False, values=False, n_valid=None):
    """Greedy acting by the definition of include/stackrl_greedy.h (`greedy_head_reference`): actions [B], then as asked
    stats [B, 4] float64 {max, min, sum, sum of squares of Q(s, .)} and Q [B, G * A].  inputs[1] may be the Stack-v2 layout
    [B, G, h, w, 1] (G object maps per env, the first `n_valid` valid; the action is row * A + pixel).  With a `policy_op`
    that has `.greedy` (qops.FusedPolicy) the rollout kernels run and no Q tensor exists unless `values` asks for it;
    otherwise the module's own pieces followed by the definition in torch (any device)."""
    timer = self.policy_timer
    if timer is not None:
      timer.start()
    try:
      if hasattr(self._policy_op, 'greedy'):
        return self._policy_op.greedy(self._q_net, inputs, n_valid=n_valid, stats=stats, values=values)
      a, st, q = self._greedy_module(inputs, n_valid)
      out = (a,) + ((st,) if stats else ()) + ((q.reshape(q.shape[0], -1),) if values else ())
      return out if len(out) > 1 else a
    finally:
      if timer is not None:
        timer.stop()

  def _greedy_module(self, inputs, n_valid):
    net = self._q_net
    xm, xo = inputs
    B = xm.shape[0]
    G = xo.shape[1] if xo.dim() == 5 else 1
    if xo.dim() == 5:      # the reference's layout (env.py:472-480): the overhead map once per object map
      inputs = (xm[:, None].expand(B, G, *xm.shape[1:]).reshape(B * G, *xm.shape[1:]), xo.reshape(B * G, *xo.shape[2:]))
    if not all(hasattr(net, k) for k in ('features', 'correlation', '_pos')):
      return greedy_head_reference(net(inputs).reshape(B, G, -1), None, n_valid)     # an opaque module: Q is what it returns
    x, x0, w = net.features(inputs)
    adv = net._pos(net.correlation(x, w)).flatten(1).reshape(B, G, -1)
    v = None
    if getattr(net, 'dueling', False):
      x0 = x0.reshape(B, G, *x0.shape[1:])[:, 0]
      v = net.value(x0.mean(dim=(2, 3)) if net.dueling_avg_pool else x0.amax(dim=(2, 3))).reshape(B)
    return greedy_head_reference(adv, v, n_valid)

  def acknowledge_reset(self):
    self._replay_memory.set_terminal()               # dqn.py:381-385

  def observe(self, state, reward, terminal, action):
    self._replay_memory.add(state, reward, terminal, action)

  def collect(self, state, reward, terminal):
    action = self.policy(state, exploration=True)
    self._replay_memory.add(state, reward, terminal, action)
    return action

  # ------------------------------------------------------------------ train (dqn.py:397-486)
  def td_targets(self, rewards, next_states, terminal):
    """y = r + where(terminal, 0, gamma * Q_target(s', argmax_a Q(s', a)))  (dqn.py:418-454)."""
    with torch.no_grad():
      if self._reward_scale is not None:
        rewards = rewards * self._reward_scale
      if self._gamma == 0 and not self._n_step:
        return rewards
      tq = self._target_q_net(next_states)
      if self._double:
        a = torch.argmax(self._q_net(next_states), dim=-1)
        tq = tq.gather(1, a[:, None])[:, 0]
      else:
        tq = tq.amax(dim=-1)
      if self._n_step:
        rewards = (self._gamma_r * rewards).sum(dim=-1)
      return rewards + torch.where(terminal, torch.zeros_like(tq), self._gamma * tq)

  def loss_from_td(self, td_abs, weights=None):
    if self._huber:
      quadratic = torch.clamp(td_abs, max=self._huber_delta)
      linear = td_abs - quadratic
      loss = 0.5 * quadratic ** 2 + self._huber_delta * linear       # dqn.py:461-464
    else:
      loss = 0.5 * td_abs ** 2
    if weights is not None:
      loss = loss * weights
    return loss.mean()

  def _draw(self):
    """One minibatch from the replay memory as a flat tuple of tensors:
    (indexes | None, weights | None, states..., actions, rewards, next_states..., terminal)."""
    if self._prioritized:
      indexes, weights, (states, actions, rewards, next_states, terminal) = \
        self._replay_memory.sample(self._minibatch_size, get_weights=True)
    else:
      indexes = weights = None
      states, actions, rewards, next_states, terminal = self._replay_memory.sample(self._minibatch_size)
    return (indexes, weights) + tuple(states) + (actions, rewards) + tuple(next_states) + (terminal,)

  def _next_minibatch(self):
    """`next(self._replay_memory_iter)` (dqn.py:399-405): the oldest minibatch of the FIFO, which then moves on
    (`MinibatchFifo`), or a fresh draw without prefetch."""
    if self._fifo is None:
      return self._split_minibatch(self._draw())
    self._fifo.fill()
    flat = self._fifo.head()
    self._fifo.advance()
    return self._split_minibatch(flat)

  @staticmethod
  def _split_minibatch(flat):
    indexes, weights = flat[0], flat[1]
    ns = (len(flat) - 5) // 2
    states, actions, rewards = flat[2:2 + ns], flat[2 + ns], flat[3 + ns]
    next_states, terminal = flat[4 + ns:4 + 2 * ns], flat[4 + 2 * ns]
    return indexes, weights, (states, actions, rewards, next_states, terminal)

  # ---- the four stages of an update (`update_plan`)
  def _grad(self):
    """Stage `grad` (dqn.py:397-469): the minibatch (a copy of the FIFO's head, which stays; a fresh draw without prefetch),
    target evaluations, forward, loss, backward into the flat gradient bucket.  Draws no random numbers with prefetch and
    writes neither the replay memory nor the FIFO.  Returns (loss, mean TD error, indexes, |TD|, new priorities or None)."""
    indexes, weights, (states, actions, rewards, next_states, terminal) = \
      self._split_minibatch(self._draw() if self._fifo is None else self._fifo.head())
    if not self._bias_compensation:
      weights = None
    self._last_sample_indexes = indexes
    if not self._fused or (self._gamma == 0 and not self._n_step):
      y = self.td_targets(rewards, next_states, terminal)
      q = self._q_net(states).gather(1, actions[:, None])[:, 0]      # one_hot . sum, dqn.py:410-417
      td = q - y
      td_abs = td.abs()
      loss = self.loss_from_td(td_abs, weights)
      self._flat_grad.zero_()
      loss.backward()
      return loss.detach(), td.mean().detach(), indexes, td_abs.detach(), None
    # target evaluations, then loss, mean TD, |TD|, new priorities and d loss / d Q(s, .) in one kernel (dqn.py:408-469)
    from stackrl_amd import qops
    if self._n_step:
      rewards = (self._gamma_r * rewards).sum(dim=-1)
    q_all, qo, tq = self._evaluate(states, next_states)
    loss, mtd, td_abs, new_logits, grad_q = qops.td_epilogue(
      q_all.detach(), qo, tq, actions, rewards, terminal, weights, self._gamma, self._huber_delta, self._reward_scale,
      self._double, self._replay_memory.epsilon, self._ws)
    if self._hand is None:
      self._flat_grad.zero_()
      q_all.backward(grad_q)
    elif self._hand_cover_checked or torch.cuda.is_current_stream_capturing():
      # no zero-fill of the gradient bucket: the hand-written backward writes every element of every parameter's gradient
      # (tests/test_train_conv_gpu.py starts it from NaN); the alignment padding between parameters keeps its initial zeros
      self._hand.backward(grad_q)
    else:
      self._hand_backward_checking_cover(grad_q)
    return loss, mtd, indexes, td_abs, new_logits

  def _evaluate(self, states, next_states):
    """(Q(s, .) to differentiate, Q(s', .) of the online net without grad or None (not double), Q_target(s', .))."""
    if self._hand is None:
      with torch.no_grad():
        tq = self._target_q_net(next_states)
        qo = self._q_net(next_states) if self._double else None
      return self._q_net(states), qo, tq
    # hand-written convolutions: Q_target(s', .), then Q(s, .) and Q(s', .) of the online net in ONE pass over the 2 mb
    # samples (activations saved; the backward runs over the first mb)
    self._hand.refresh()
    with torch.no_grad():
      tq = self._hand_t.forward(next_states)
    if not self._double:
      return self._hand.forward(states, save=True), None, tq
    mb = int(states[0].shape[0])
    q2 = self._hand.forward(tuple(torch.cat([a, b]) for a, b in zip(states, next_states)), save=True)
    return q2[:mb], q2[mb:].detach(), tq

  def _hand_backward_checking_cover(self, grad_q):
    """Once, on the first eager update: every parameter's gradient starts from NaN, so that a parameter the hand-written
    backward does not write (a layer HandNet does not cover, a frozen or non-dueling variant) cannot keep the previous
    step's — or, with several ranks, the previously all-reduced — value unnoticed."""
    for p in self._q_net.parameters():
      p.grad.fill_(float('nan'))
    self._hand.backward(grad_q)
    self._hand_cover_checked = True
    missed = [n for n, p in self._q_net.named_parameters() if not bool(torch.isfinite(p.grad).all())]
    if missed:
      raise RuntimeError('HandNet.backward left (part of) these gradients unwritten: {}'.format(missed))

  def _apply(self, indexes, td_abs, new_logits):
    """Stage `apply` (dqn.py:470-476): average over the ranks, optimiser step, new replay priorities."""
    if self._world > 1:
      self._flat_grad.div_(self._world)
    if isinstance(self._optimizer, KerasAdam):
      self._optimizer.step(self._flat_grad)
    else:
      self._optimizer.step()
    if self._prioritized:
      self._replay_memory.update_priorities(indexes, td_abs, logits=new_logits)   # dqn.py:475-476

  def _stage(self, name):
    if name == 'grad':
      self._out = self._grad()
    elif name == 'fifo':
      self._fifo.advance()
    elif name == 'reduce':
      # the one collective of the update: the flat gradient bucket summed over the ranks (RCCL over xGMI)
      dist.all_reduce(self._flat_grad, op=dist.ReduceOp.SUM, group=self._pg)
    else:
      self._apply(*self._out[2:])

  # ---- where the stages run
  _GRAPH_WARMUP = 3   # eager updates before the capture (library solver search, optimiser state, lazy initialisations)

  @property
  def _train_graph(self):
    """The first hipGraph of the serial update, once captured."""
    return None if self._early else self._captured.get(0)

  @property
  def _grad_graph(self):
    """The hipGraph of `grad` on the update stream (`early_gradient`), once captured."""
    return self._captured.get(0) if self._early else None

  def _run_segment(self, plan, i):
    """Segment i of `plan`: its stages one after the other, or — a graphed segment — their replay from one hipGraph, which
    is captured on first use: all graphs in the first one's pool, the sampling generator registered with the one that draws,
    `grad`'s outputs handed on as the captured tensors themselves."""
    seg = plan[i]
    if not seg.graph:
      for name in seg.stages:
        self._stage(name)
      return
    g = self._captured.get(i)
    if g is None:
      mem = self._replay_memory
      mem.tensor_schedules = True            # the graph reads alpha / beta from the scalars `refresh_schedules` writes
      g = torch.cuda.CUDAGraph()
      if seg.draws:
        g.register_generator_state(mem._gen)
      with torch.cuda.graph(g, pool=self._captured[0].pool() if i else None, capture_error_mode=CAPTURE_MODE,
                            stream=self._upd_stream if seg.stream == 'update' else None):
        for name in seg.stages:
          self._stage(name)
      self._captured[i] = g
    g.replay()

  def _start(self):
    """What stays eager and comes before the stages, then the first segment of the update."""
    if self._hand_t is not None:
      self._hand_t.refresh_if_stale()          # outside any graph: the target net changes only through framework ops
    if self._graphs:
      self._replay_memory.refresh_schedules()
    if self._fifo is not None:
      self._fifo.fill()
    plan = self._plan if self._updates >= self._warmup else self._warmup_plan
    if plan[0].stream == 'update':
      main, upd = torch.cuda.current_stream(self.device), self._upd_stream
      upd.wait_stream(main)                    # the weights of the previous update, the FIFO as the previous train() left it
      with torch.cuda.stream(upd):
        self._run_segment(plan, 0)
        if not plan[0].graph:
          for t in self._out:
            if torch.is_tensor(t):
              t.record_stream(main)            # allocated on the update stream, consumed by train() on the current one
    else:
      self._run_segment(plan, 0)
    self._running = plan

  def train_begin(self):
    """Start the gradient half of the next update beside the collect step (see `early_gradient`).  Call it before
    `collect` / `Trainer.collect_step`; `train()` completes the update.  Returns whether anything was started.  (The first
    update fills the FIFO from the replay memory and the warm-up updates of `graphs` are serial: nothing to start.)"""
    if not self._early or self._running is not None or self._fifo.slots is None or self._updates < self._warmup:
      return False
    self._start()
    return True

  def train(self):
    if self._running is None:
      self._start()
    plan, self._running = self._running, None
    if plan[0].stream == 'update':
      torch.cuda.current_stream(self.device).wait_stream(self._upd_stream)
    for i in range(1, len(plan)):
      self._run_segment(plan, i)
    loss, mtd = self._out[:2]
    if plan[0].graph:
      loss, mtd = loss.clone(), mtd.clone()    # the graph's own tensors: the next replay overwrites them
    self._updates += 1
    self._iterations += 1
    # consumers that cache re-packed weights (qops.FastFeatures) key on this: a graph replay changes the parameters
    # without bumping any tensor version
    self._q_net._weights_epoch = getattr(self._q_net, '_weights_epoch', 0) + 1   # monotonic: bumped by every update and every restore
    if self._iterations % self._target_update_period == 0:           # dqn.py:478-484
      self._target_q_net.load_state_dict(self._target_sync_source())
      if self._hand_t is not None:
        self._hand_t.refresh()                                       # eagerly: the target's packed weights are read by the graph
    return loss, mtd

  def _target_sync_source(self):
    return self._q_net.state_dict()

  def save_weights(self, path):
    torch.save(self._q_net.state_dict(), path)

  def state_dict(self, memory=True):
    """Everything `tf.train.Checkpoint(agent=...)` tracks in the reference (training.py:199-208): both nets, the
    optimiser slots, the iteration counter, the RNG stream and (optionally) the replay memory."""
    d = {'q_net': self._q_net.state_dict(), 'target_q_net': self._target_q_net.state_dict(),
         'optimizer': self._optimizer.state_dict(), 'iterations': int(self._iterations), 'gen': self._gen.get_state()}
    if memory:
      d['replay_memory'] = self._replay_memory.state_dict()
      # the minibatches already drawn and waiting (`dataset.prefetch`, dqn.py:247-252): part of the state, or a resumed run
      # would train on freshly drawn ones where the uninterrupted run trains on these
      if self._fifo is not None and self._fifo.slots is not None:
        d['prefetched'] = self._fifo.state()
    return d

  def load_state_dict(self, d):
    """Accepts the whole dict of `state_dict` or a part of it (the Trainer keeps what the replicas share and what belongs
    to one rank in separate files)."""
    if 'q_net' in d:
      self._q_net.load_state_dict(d['q_net'])
      self._target_q_net.load_state_dict(d['target_q_net'])
      self._optimizer.load_state_dict(d['optimizer'])
      self._iterations = int(d['iterations'])
      self._q_net._weights_epoch = getattr(self._q_net, '_weights_epoch', 0) + 1   # restored weights: a new epoch, never an earlier one's
      if self._hand_t is not None:
        self._hand_t.refresh()
    if self._running is not None:
      # a gradient half computed from the weights / minibatch being replaced is in flight on the update stream: wait for
      # it and drop it (the next train() starts over from the restored state)
      torch.cuda.current_stream(self.device).wait_stream(self._upd_stream)
      self._running = None
    if 'gen' in d:
      self._gen.set_state(d['gen'].cpu())
    if 'replay_memory' in d:
      self._replay_memory.load_state_dict(d['replay_memory'])
      if self._fifo is not None:
        self._fifo.load(d.get('prefetched'), captured=bool(self._captured))

  def reseed(self, seed):
    """New streams for exploration and minibatch sampling (a rank that resumes without state of its own)."""
    self._gen.manual_seed(int(seed) % (2 ** 63) + 1)
    self._replay_memory._gen.manual_seed(int(seed) % (2 ** 63))