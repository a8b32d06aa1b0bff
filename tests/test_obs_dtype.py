"""CPU tests of the observation dtypes (env.py:24, :168-180): the seven names of the reference, their C enum and how the
configuration carries them; the guards that keep other dtypes away from the uint8-only learner kernels."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('uint8', 'uint16', 'uint32', 'uint64', 'float16', 'float32', 'float64')   # env.py:24, in its order


def _header_enum():
  with open(os.path.join(ROOT, 'include', 'srl_types.h')) as f:
    txt = f.read()
  return {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'\bSRL_DTYPE_([A-Z0-9]+)\s*=\s*(\d+)', txt)}


def test_config_accepts_the_seven_reference_dtypes_and_maps_them_to_the_enum():
  from stackrl_amd.config import StackConfig
  enum = _header_enum()
  assert sorted(enum) == sorted(NAMES)
  for k, name in enumerate(NAMES):
    c = StackConfig(dtype=name)
    assert c.dtype == name
    assert c.to_c().obs_dtype == enum[name] == k
  assert StackConfig().to_c().obs_dtype == enum['uint8']          # the registry's Stack-v0 value (and the class default here)


@pytest.mark.parametrize('bad', ['int8', 'float33', 'bfloat16', 'uint'])
def test_config_rejects_other_dtypes_like_the_reference(bad):
  from stackrl_amd.config import StackConfig
  with pytest.raises(ValueError, match='Invalid value {} for argument dtype'.format(bad)):   # env.py:169-170
    StackConfig(dtype=bad)


def test_python_tables_agree_with_the_header():
  from stackrl_amd import config
  assert config.DTYPES == _header_enum()
  assert config.CConfig._fields_[-1][0] == 'obs_dtype'            # appended: the fields before it keep their offsets
  torch = pytest.importorskip('torch')
  from stackrl_amd import env
  assert sorted(env.TORCH_DTYPES) == sorted(NAMES)
  for name, dt in env.TORCH_DTYPES.items():
    assert dt == getattr(torch, name)


def test_env_path_names_the_dtype():
  from stackrl_amd import env
  assert 'dtypuint8' in env.env_path('Stack-v0')
  p = env.env_path('Stack-v0', dtype='float32')
  assert 'dtypfloat32' in p and 'dtypuint8' not in p
  assert 'dtypuint16' in env.env_path('Stack-v1', dtype='uint16')


def test_heuristics_refuse_other_dtypes_before_any_device_work():
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines
  for dt in (torch.float32, torch.uint16):
    xm = torch.zeros((2, 128, 128, 2), dtype=dt)                   # CPU tensors: the dtype check comes first
    xo = torch.zeros((2, 32, 32, 1), dtype=dt)
    with pytest.raises(ValueError, match=str(dt).replace('torch.', '')):
      baselines.heuristic_values('height', (xm, xo))


def test_training_refuses_an_env_with_other_dtypes():
  torch = pytest.importorskip('torch')
  from stackrl_amd.env import TensorSpec
  from stackrl_amd.training import Trainer

  class Spec(object):       # only what Trainer reads before it touches the agent
    def __init__(self, dt):
      self.observation_spec = (TensorSpec((128, 128, 2), dt), TensorSpec((32, 32, 1), dt))
      self.batch_size = 2

  with pytest.raises(ValueError, match='float32'):
    Trainer(Spec(torch.float32), agent=None)
  with pytest.raises(ValueError, match='uint64'):
    Trainer(Spec(torch.uint8), agent=None, eval_env=Spec(torch.uint64))


def test_stack_v1_default_start_policy_needs_uint8():
  pytest.importorskip('torch')
  from stackrl_amd import env
  with pytest.raises(ValueError, match='uint16'):     # raised before the handle is created (no device needed)
    env.make('Stack-v1', n_parallel=2, episode_length=3, n_objects=5, dtype='uint16')
