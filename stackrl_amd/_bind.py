"""The ctypes binding the native libraries share: one loader and one checked launch per library of `build.LIBRARIES`.
Each wrapper module (lib.py, qops.py, compare.py, rocks.py, valueview.py, candidates.py) keeps its signature table and gets
`load` and `call` from here."""
import ctypes
import os

import torch

from stackrl_amd import build as _build


def stream(t):
  return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def binding(library, sigs):
  """(`load`, `call`) of `build.LIBRARIES[library]`. `sigs`: export -> (restype, argtypes[, error accessor or None])."""
  loaded = None

  def load():
    """Load (building first if the library is missing) and return the ctypes library; a symbol of `_SIGS` it lacks fails here."""
    nonlocal loaded
    if loaded is None:
      path = _build.LIBRARIES[library].path   # read now, not at import: a diagnostic may have pointed it at another build
      if not os.path.isfile(path):
        _build.build()
      lib = ctypes.CDLL(path)
      for name, sig in sigs.items():
        fn = getattr(lib, name)  # AttributeError = symbol missing: fail loudly
        fn.restype, fn.argtypes = sig[0], sig[1]
      loaded = lib
    return loaded

  def call(name, t, *args):
    """One launch of the export `name` on the device and current stream of tensor `t`: tensors among `args` go as their
    data pointers, None as NULL, the stream last; a non-zero return raises RuntimeError with the text of the export's own
    error accessor (`_SIGS`)."""
    lib = load()
    with torch.cuda.device(t.device):
      rc = getattr(lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], stream(t))
    if rc:
      raise RuntimeError(getattr(lib, sigs[name][2])().decode())

  return load, call
