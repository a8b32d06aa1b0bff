"""GPU test of the Q-net binding's checked call (`qops.call`): a launch the host code refuses reaches the caller as a
RuntimeError with the text of the refusing file's own error buffer.  One export per buffer, each through its Python wrapper,
each refused by the launcher's argument check before anything is launched (tests/test_abi.py holds the table's pairing of
export and accessor to the sources on the CPU)."""
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

_CL = torch.channels_last


def _qnet():          # csrc/heuristics.hip (srl_qnet_last_error): methods are 1..4
  from stackrl_amd import baselines
  xm = torch.zeros((1, 16, 16, 2), dtype=torch.uint8, device='cuda')
  xo = torch.zeros((1, 4, 4, 1), dtype=torch.uint8, device='cuda')
  baselines.heuristic_values(9, (xm, xo))


def _xcorr():         # csrc/xcorr_mfma.hip: precisions are 0 and 1
  from stackrl_amd import qops
  x = torch.zeros((1, 1, 64, 64), dtype=torch.bfloat16, device='cuda')
  w = torch.zeros((1, 1, 16, 16), dtype=torch.bfloat16, device='cuda')
  qops.xcorr_forward_mfma(x, w, precision=2)


def _epilogue():      # csrc/epilogue.hip: 12 channels are no multiple of 8
  from stackrl_amd import qops
  y = torch.zeros((1, 12, 4, 4), dtype=torch.bfloat16, device='cuda').contiguous(memory_format=_CL)
  qops.bias_act(y, torch.zeros(12, device='cuda'))


def _conv():          # csrc/conv_mfma.hip: the pooled output and the NCHW store exclude each other
  from stackrl_amd import qops
  x = torch.zeros((1, 16, 16, 16), dtype=torch.bfloat16, device='cuda').contiguous(memory_format=_CL)
  w = qops.pack_conv3x3_weights(torch.zeros(16, 16, 3, 3, device='cuda'))
  qops.conv3x3_bias_relu(x, w, torch.zeros(16, device='cuda'), 16, pool=True, nchw=True)


def _conv_gemm():     # csrc/conv_gemm.hip: 32 -> 64 channels at 4 x 4 is no layer of srl_conv3x3_gemm_supported
  from stackrl_amd import qops
  assert not qops.load().srl_conv3x3_gemm_supported(32, 64, 4)
  x = torch.zeros((1, 32, 4, 4), dtype=torch.bfloat16, device='cuda').contiguous(memory_format=_CL)
  qops.conv3x3_gemm_bias_relu(x, torch.zeros(8, dtype=torch.bfloat16, device='cuda'), torch.zeros(64, device='cuda'), 64)


def _learner():       # csrc/learner.hip: a parameter bucket that starts 4 bytes past a 16-byte boundary
  from stackrl_amd import qops
  buf, z = torch.zeros(8, device='cuda'), [torch.zeros(4, device='cuda') for _ in range(4)]
  assert buf.data_ptr() % 16 == 0
  qops.adam_step(buf[1:5], z[0], z[1], z[2], z[3], 1e-3, 0.9, 0.999, 1e-7)


def _train_conv():    # csrc/train_conv.hip: 8 output channels are no multiple of 16
  from stackrl_amd import qtrain
  x = qtrain.Act(torch.zeros((1, 2, 2, 4), device='cuda'))
  qtrain.tconv(x, torch.zeros(9 * 4 * 8, device='cuda'), None, 8)


REFUSALS = [('srl_qnet_last_error', _qnet, 'srl_heuristic: bad arguments'),
            ('srl_xcorr_mfma_last_error', _xcorr, 'srl_xcorr_mfma: bad arguments'),
            ('srl_epilogue_last_error', _epilogue, 'srl_bias_act: bad arguments'),
            ('srl_conv_last_error', _conv, 'srl_conv3x3_bias_relu: bad arguments'),
            ('srl_conv_gemm_last_error', _conv_gemm, 'srl_conv3x3_gemm_bias_relu: bad arguments'),
            ('srl_learner_last_error', _learner, 'srl_adam_step: buffers must be 16-byte aligned'),
            ('srl_train_conv_last_error', _train_conv, 'srl_tconv: bad arguments')]


def test_one_refusal_per_error_buffer():
  from stackrl_amd import qops
  assert sorted(r[0] for r in REFUSALS) == sorted({err for _, _, err in qops._SIGS.values() if err})


@pytest.mark.parametrize('accessor,refused,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_launch_raises_its_own_files_message(accessor, refused, message):
  """The wrapper raises RuntimeError, the text names the refusing export (another file's buffer, stale or empty, would not),
  and it is what that file's accessor returns."""
  from stackrl_amd import qops
  with pytest.raises(RuntimeError) as e:
    refused()
  assert str(e.value).startswith(message)
  assert getattr(qops.load(), accessor)().decode() == str(e.value) != ''
  torch.cuda.synchronize()
