"""ctypes loader of libstackrl_hip.so (include/stackrl_hip.h): `load` builds first if the library is missing and returns the
ctypes library.  There is no CPU fallback: if the HIP library is missing or cannot be loaded the import of the product path
fails loudly."""
import ctypes

from stackrl_amd import _bind, build as _build
from stackrl_amd.config import CConfig

_VP = ctypes.c_void_p
_SIGS = {
  'srl_config_default': (ctypes.c_int, [ctypes.POINTER(CConfig)]),
  'srl_create': (ctypes.c_int, [ctypes.POINTER(CConfig), ctypes.POINTER(_VP)]),
  'srl_destroy': (None, [_VP]),
  'srl_last_error': (ctypes.c_char_p, []),
  'srl_load_meshes': (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, ctypes.c_int32]),
  'srl_seed': (ctypes.c_int, [_VP, ctypes.c_uint32]),
  'srl_set_script': (ctypes.c_int, [_VP, _VP, _VP]),
  'srl_reset': (ctypes.c_int, [_VP, _VP, _VP, _VP]),
  'srl_step': (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
  'srl_sample': (ctypes.c_int, [_VP, _VP, _VP]),
  'srl_sync_status': (ctypes.c_int, [_VP, _VP]),
  'srl_get_state': (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP]),
  'srl_get_maps': (ctypes.c_int, [_VP, _VP, _VP, _VP]),
  'srl_get_velocities': (ctypes.c_int, [_VP, _VP]),
  'srl_get_sweeps': (ctypes.c_int, [_VP, _VP]),
  'srl_set_body_state': (ctypes.c_int, [_VP, _VP, _VP]),
  'srl_step_simulation': (ctypes.c_int, [_VP, ctypes.c_int32, _VP]),
  'srl_get_contacts': (ctypes.c_int, [_VP, _VP, _VP]),
  'srl_render_heightmap': (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
  'srl_get_object_map': (ctypes.c_int, [_VP, ctypes.c_int32, _VP]),
  'srl_render_rgb': (ctypes.c_int, [_VP, ctypes.c_int32, _VP, _VP, _VP]),
  'srl_render_camera': (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
  'srl_set_profiling': (ctypes.c_int, [_VP, ctypes.c_int32]),
  'srl_get_kernel_times': (ctypes.c_int, [_VP, _VP, _VP]),
  'srl_get_order_kernel_times': (ctypes.c_int, [_VP, _VP, _VP]),
  'srl_get_launch_order': (ctypes.c_int, [_VP, _VP, _VP]),
  'srl_set_concurrent_envs': (ctypes.c_int, [_VP, ctypes.c_int32]),
  'srl_get_step_variant': (ctypes.c_int, [_VP, _VP, _VP, _VP]),
  'srl_set_launch_order': (ctypes.c_int, [_VP, ctypes.c_int32]),
  'srl_build_info': (ctypes.c_char_p, []),
  'srl_get_stage_records': (ctypes.c_int, [_VP, _VP, ctypes.c_int64]),
  'srl_stage_record_stride': (ctypes.c_int32, []),
  'srl_state_layout': (ctypes.c_int, [ctypes.POINTER(CConfig), _VP, _VP]),
  'srl_state_signature': (ctypes.c_int, [_VP, _VP]),
  'srl_state_get': (ctypes.c_int, [_VP, _VP, ctypes.c_int32, _VP, _VP, _VP, _VP]),
  'srl_state_set': (ctypes.c_int, [_VP, ctypes.c_uint64, _VP, _VP, ctypes.c_int32, _VP, _VP]),
  'srl_state_set_rng': (ctypes.c_int, [_VP, ctypes.c_uint32, ctypes.c_uint32]),
  'srl_contact_row_words': (ctypes.c_int32, []),
  'srl_contact_max_points': (ctypes.c_int, [_VP, _VP]),
  'srl_contact_points': (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_int32, _VP, _VP, _VP, _VP, _VP]),
  'srl_poses': (ctypes.c_int, [_VP, _VP, _VP, _VP]),
  'srl_kick': (ctypes.c_int, [_VP, _VP, ctypes.c_int32, ctypes.c_int32, _VP]),
  'srl_pose_distances': (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_float, ctypes.c_float, _VP, _VP, _VP]),
}
EXPORTS = tuple(sorted(_SIGS))


load, _ = _bind.binding('env', _SIGS)      # the handle API reports its errors per call (env.py `_check`), not through `call`


def path():
  return _build.LIBRARIES['env'].path


def last_error():
  return load().srl_last_error().decode()
