"""The frequency case shared by tests/test_boltzmann.py (the torch restatement) and tests/test_boltzmann_gpu.py (the kernel):
five actions, 65,536 seeded stream keys, the binomial bound."""
import torch

FREQ_ADV = (0.3, -1.2, 1.0, 0.0, 0.55)
FREQ_T = 0.7
FREQ_N = 65536


def freq_keys(device='cpu'):
  return torch.randint(0, 2 ** 32, (FREQ_N, 2), dtype=torch.int64, generator=torch.Generator().manual_seed(11)).to(device)


def check_frequencies(actions):
  """Every action's frequency within 5 standard deviations, 5 sqrt(p (1 - p) / N), of p = softmax(adv / T): the binomial bound
  (about 3e-6 false alarms per action, and none or one for good once the seed is fixed)."""
  p = torch.softmax(torch.tensor(FREQ_ADV, dtype=torch.float64) / FREQ_T, dim=0)
  assert actions.shape == (FREQ_N,) and int(actions.min()) >= 0 and int(actions.max()) < len(FREQ_ADV)
  f = torch.bincount(actions.cpu(), minlength=len(FREQ_ADV)).double() / FREQ_N
  sigma = torch.sqrt(p * (1 - p) / FREQ_N)
  print('deviations from softmax(adv / T) in standard deviations:', ((f - p) / sigma).tolist())
  assert bool(((f - p).abs() <= 5 * sigma).all()), ((f - p) / sigma).tolist()
