"""The state record's layout, restated from its definition (include/stackrl_hip.h "State records"; csrc/state.hip), for
tests/test_state_layout.py: a record is an env's header, its blob words, its height map and its staged render records, each
part padded to a multiple of 4 words.  The blob is restated as `layout()` of csrc/stackrl_hip.hip builds it, `nslots` as that
file defines it; the word constants are read from the `#define`s of csrc/srl_device.h and csrc/stage.h."""
import os
import re

from stackrl_amd import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'stackrl_amd', 'csrc')
_DEFINE = re.compile(r'^[ \t]*#[ \t]*define[ \t]+(SRL_\w+)[ \t]+([^\n]*?)[ \t]*(?://[^\n]*|/\*[^\n]*)?$', re.M)


def defines(*paths):
  """{name: int} of the object-like `#define SRL_...` lines of the files whose value is integer arithmetic on earlier ones."""
  out = {}
  for p in paths:
    with open(p) as f:
      for name, expr in _DEFINE.findall(f.read()):
        if re.fullmatch(r'[\w\s()+*\-]+', expr or '') and not re.search(r'\d[A-Za-z]|\.', expr):
          try:
            out[name] = int(eval(expr, {'__builtins__': {}}, dict(out)))
          except Exception:
            pass
  return out


D = defines(os.path.join(ROOT, 'include', 'srl_types.h'), os.path.join(CSRC, 'srl_device.h'), os.path.join(CSRC, 'stage.h'))

# EnvHdr (csrc/srl_kernels.h), field by field, in 32-bit words: nb, done, episode, list_pos, pending, mode; goal[4];
# prev_metric[4]; substeps[2]; sweeps, status, ncolour, has_script; ids[MAX_BODIES]; script_ids[MAX_BODIES]; script_goal[4]
HDR_WORDS = 6 + 4 + 4 + 2 + 4 + 2 * config.MAX_BODIES + 4


def nslots(L):
  """Manifold slots per env: every pair up to the cap of 64 (up to 16 rocks) or 128."""
  pairs = max(L * (L - 1) // 2, 1)
  return min(pairs, 64 if L <= 16 else 128)


def blob_words(L):
  NS, NP = nslots(L), max(L * (L - 1) // 2, 1)
  o = 8 * L                       # velocities, interleaved
  o += 4 * L * 4                  # X, Q, PX, PQ
  o += L                          # mesh ids
  o += D['SRL_GM_WORDS'] * L      # ground manifolds
  o += D['SRL_MAN_WORDS'] * NS    # pair manifolds
  o += NP                         # slot of pair
  o += 2 * NS                     # pair of slot, colour
  return (o + 3) & ~3


def pad4(w):
  return (w + 3) & ~3


def expected(L, resolution_factor, observable_size_ratio, stride):
  """(words, [offset of header, blob, height map, staged records]); `stride` = srl_stage_record_stride()."""
  res = 2 ** resolution_factor * observable_size_ratio
  sizes = [pad4(HDR_WORDS), pad4(blob_words(L)), pad4(res * res), pad4(L * stride * 4)]
  off = [sum(sizes[:k]) for k in range(4)]
  return sum(sizes), off
