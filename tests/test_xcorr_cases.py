"""The operands and expectations of tests/xcorr_cases.py, without a GPU.

  * Every case of tests/test_xcorr_exact_gpu.py meets the condition that makes its float64 result the only float32 answer: the
    sum of its terms' magnitudes is at most 2^22 units at every output (a condition the builders assert, not a measurement).
  * The host's split returns exactly the (h, l) planes the split operands were built from.
  * Every map position and every tap position of a case carries a value (a lo part, in the split cases) in some sample and
    channel, and no two samples of a case are alike.
  * The expectations are right: `corr64` against `nets.correlation_reference` and its autograd gradients at both geometries,
    and against a plain numpy loop on a small case.
  * The cases have teeth: the restatement with one deliberate defect at a time — one tap read a column off, the lo plane of
    the map's last column zeroed, one channel dropped, truncation instead of round-to-nearest-even — differs from the
    expectation of every case whose path has that failure mode (for the rounding case: by more than 10 x its tolerance)."""
import pytest

import xcorr_cases as XC

torch = pytest.importorskip('torch')

import test_xcorr_exact_gpu as TX           # noqa: E402  (parameter lists only; nothing in them runs at import)


def exact_cases():
  """(builder, B, C, H, h, modes) of every exact case the GPU file runs."""
  out = []
  for H, h in TX.GEOMETRIES:
    out += [(XC.int_case, B, C, H, h, (0, 1, 2)) for B, C in TX.TOEPLITZ_BC]
    out += [(XC.split_case, B, C, H, h, (0, 1, 2)) for B, C in TX.SPLIT_BC]
    out += [(f, TX.LARGE_DISTINCT, 16, H, h, (0,)) for f in (XC.int_case, XC.split_case)]
  for f in (XC.int_case, XC.split_case):
    out += [(f, 3, C, 128, 32, (0,)) for C in TX.ROWS_CHANNELS]
    out += [(f, B, C, 128, 32, (0,)) for B, C in TX.ROWS_ENTRY_BC]
  seen, uniq = set(), []
  for c in out:
    if c[:5] not in seen:
      seen.add(c[:5]); uniq.append(c)
  return uniq


EXACT = exact_cases()
SMALL = [c for c in EXACT if c[1] <= TX.LARGE_DISTINCT]        # the defects are restated on these: a 32-sample case is its 3-sample one's kernel paths
_id = lambda c: '%s-%d-%d-%d-%d' % ((c[0].__name__,) + c[1:5])


@pytest.mark.parametrize('case', EXACT, ids=_id)
def test_every_sum_of_every_case_is_a_float32_value(case):
  f, B, C, H, h, modes = case
  c = f(B, C, H, h)
  for mode in modes:
    e = XC.expect(c, mode)                  # asserts the condition and that the result is a float32 value in whole units
    assert c['bound'][mode] <= 2.0 ** 22 and float(e.abs().max()) <= c['bound'][mode] * c['lsb']
    assert float(e.abs().max()) > 0
  # the hand-worked limits of the integer operands
  if f is XC.int_case:
    assert C * h * h * 6 <= 16384 * 6 < 2 ** 17 and (H - h + 1) ** 2 * 6 <= 9409 * 6 < 2 ** 16


@pytest.mark.parametrize('case', [c for c in EXACT if c[0] is XC.split_case], ids=_id)
def test_the_host_split_returns_the_planes_the_operands_were_built_from(case):
  f, B, C, H, h, _ = case
  c = f(B, C, H, h)
  for name, (hi, lo) in c['parts'].items():
    got_hi, got_lo = XC.split_bf16(c[name])
    assert torch.equal(got_hi, hi) and torch.equal(got_lo, lo), name
    assert torch.equal(hi, hi.round()) and float(hi.abs().max()) <= 2
    assert set((lo / XC.LO).unique().tolist()) <= {-1.0, 0.0, 1.0} and not bool(((hi == 0) & (lo != 0)).any())
    assert torch.equal(c[name].double(), hi.double() + lo.double())
  assert int((c['w'] != 0).sum(dim=(2, 3)).max()) <= XC.taps_per_kernel(B, C, h)


@pytest.mark.parametrize('case', EXACT, ids=_id)
def test_every_position_is_covered_and_no_two_samples_are_alike(case):
  f, B, C, H, h, _ = case
  c = f(B, C, H, h)
  used = sorted({name for mode in case[5] for name in (('x', 'w'), ('g_dx', 'w'), ('x', 'g_dw'))[mode]})      # the operands of the case's modes
  for name in used:
    t = c['parts'][name][1] if c['split'] else c[name]                     # a lo part is non-zero only where the hi part is
    assert bool((t != 0).any((0, 1) if t.dim() == 4 else (0,)).all()), (name, 'positions without a value in any sample')
  if not c['split']:
    assert set(c['x'].unique().tolist()) == {0.0, 1.0, 2.0, 3.0} and set(c['w'].unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert {-2.0, -1.0, 1.0, 2.0} <= set(c['g_dx'].unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}    # (one sample: no zero is left)
    assert torch.equal(c['x'].bfloat16().float(), c['x']) and torch.equal(c['w'].bfloat16().float(), c['w'])
  for name in used:
    t = c[name].reshape(B, -1)
    assert all(not torch.equal(t[i], t[j]) for i in range(B) for j in range(i + 1, B)), name
  for mode in case[5]:
    e = XC.expect(c, mode).reshape(B, -1)
    assert all(not torch.equal(e[i], e[j]) for i in range(B) for j in range(i + 1, B))


@pytest.mark.parametrize('H,h', XC.GEOMETRIES)
def test_corr64_is_the_library_formulation_and_its_autograd(H, h):
  """`nets.correlation_reference` in float64 and autograd for the two gradients — bit for bit, since no sum rounds — on
  integer and on split operands."""
  from stackrl_amd import nets
  for f in (XC.int_case, XC.split_case):
    c = f(2, 3, H, h)
    for g in {id(c['g_dx']): c['g_dx'], id(c['g_dw']): c['g_dw']}.values():
      x = c['x'].double().requires_grad_(); w = c['w'].double().requires_grad_()
      ref = nets.correlation_reference(x, w)
      ref.backward(g.double()[:, None])
      assert torch.equal(ref.detach(), XC.op(0, c['x'], c['w']))
      assert torch.equal(x.grad, XC.op(1, XC.pad_gradient(g, h), XC.flip(c['w'])))
      assert torch.equal(w.grad, XC.op(2, c['x'], g))
    if f is XC.int_case:
      assert torch.equal(ref.detach().float(), XC.expect(c, 0))


def test_the_expectations_equal_plain_loops_on_a_small_case():
  """12 x 12 maps and 4 x 4 kernels: the plain loop over taps, with and without each defect, against the `corr64` forms."""
  for f in (XC.int_case, XC.split_case):
    c = f(2, 3, 12, 4)
    for mode in (0, 1, 2):
      a, k = XC.operands(c, mode)
      want = XC.expect(c, mode).double()
      assert torch.equal(XC.defective(mode, a, k, c['split'], None, loops=True), want)
      assert torch.equal(XC.defective(mode, a, k, c['split'], None), want)
      for defect in _defects_of(c, mode):
        slow, fast = XC.defective(mode, a, k, c['split'], defect, loops=True), XC.defective(mode, a, k, c['split'], defect)
        assert torch.equal(slow, fast) and not torch.equal(fast, want), (mode, defect)


def _defects_of(c, mode):
  """The failure modes a path has: any launch can misplace a tap; the forward sums channels; a split launch stages a lo plane
  of the map (the padded gradient of d/dx ends in zeros: its last column says nothing)."""
  out = [XC.DEFECTS[0]]
  if c['split'] and mode != 1:
    out.append(XC.DEFECTS[1])
  if mode == 0 and c['C'] > 1:
    out.append(XC.DEFECTS[2])
  return out


@pytest.mark.parametrize('case', SMALL, ids=_id)
def test_one_defect_at_a_time_changes_the_expectation(case):
  f, B, C, H, h, modes = case
  c = f(B, C, H, h)
  for mode in modes:
    a, k = XC.operands(c, mode)
    want = XC.expect(c, mode).double()
    for defect in _defects_of(c, mode):
      got = XC.defective(mode, a, k, c['split'], defect)
      assert not torch.equal(got, want), (mode, defect)
      assert float((got - want).abs().max()) >= c['lsb']            # a whole unit at the least: nothing a bit-for-bit test can miss


@pytest.mark.parametrize('B,C,H,h', TX.ROUNDING_FORWARD + TX.ROUNDING_GRADIENTS)
def test_truncation_moves_the_rounding_case_beyond_its_tolerance(B, C, H, h):
  """Truncated instead of rounded operands move every mode's result by far more than the 2e-5 the rounding case allows; the
  unrounded operands lie some 1e-3 away, inside the old bound of 6e-3.  (A single tap is 1e-4 to 1e-5 of a dense forward:
  misplaced taps are the exact cases' business.)"""
  c = XC.rounding_case(min(B, 3), C, H, h)
  modes = (0,) if (B, C, H, h) in TX.ROUNDING_FORWARD else (1, 2)
  for mode in modes:
    a, k = XC.operands(c, mode)
    rounded, unrounded = XC.rounding_refs(c, mode)
    assert torch.equal(XC.defective(mode, a, k, False, None), rounded)
    r = XC.ratio(XC.defective(mode, a, k, False, XC.DEFECTS[3]), rounded)
    print(mode, XC.DEFECTS[3], r)
    assert r >= 10 * XC.ROUNDING_TOL, (mode, r)
    r = XC.ratio(unrounded, rounded)
    assert XC.ROUNDING_TOL < r < 6e-3, r
