"""The camera of `render_camera` (csrc/camera.hip behind `srl_render_camera`, include/stackrl_hip.h): where the eye is, where it
looks, the light and the colours, all in Python doubles; `to_c` rounds the finished vectors to the float32 struct the kernel
reads, so the device does no trigonometry.

Convention (this build's own: pybullet is on no machine of this project, so it is not pinned to the viewer's
`resetDebugVisualizerCamera`): z is up, angles in degrees,
  fwd   = (-sin yaw * cos pitch, cos yaw * cos pitch, sin pitch)
  eye   = target - distance * fwd
  right = (cos yaw, sin yaw, 0)          (fwd x z, unit)
  up    = right x fwd
yaw 0 looks along +y, a negative pitch looks down.  `fov` is the vertical field of view."""
import ctypes
import dataclasses
import math

_V3 = ctypes.c_float * 3


class CCamera(ctypes.Structure):
  """Mirror of `srl_camera` (include/stackrl_hip.h)."""
  _fields_ = [('eye', _V3), ('fwd', _V3), ('right', _V3), ('up', _V3), ('light', _V3), ('ambient', ctypes.c_float),
              ('diffuse', ctypes.c_float), ('rock_rgb', _V3), ('sky_rgb', _V3), ('width', ctypes.c_int32),
              ('height', ctypes.c_int32), ('shadows', ctypes.c_int32)]


def _unit(v):
  n = math.sqrt(sum(x * x for x in v))
  if not n > 0:
    raise ValueError('a direction must not be the zero vector')
  return tuple(x / n for x in v)


def _cross(a, b):
  return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


@dataclasses.dataclass
class Camera:
  eye: tuple                            # world position
  fwd: tuple                            # unit viewing direction
  right: tuple                          # unit, horizontal
  up: tuple                             # unit, right x fwd
  fov: float = 60.                      # vertical field of view, degrees
  light: tuple = (-0.35, -0.45, 0.7)    # towards the light (normalised by `to_c`): about 50 degrees up, to the left of the
                                        # reference view, so that shadows fall to the right of the rocks and not behind them
  ambient: float = 0.35
  diffuse: float = 0.65
  rock_rgb: tuple = (0.62, 0.56, 0.5)
  sky_rgb: tuple = (0.55, 0.7, 0.9)
  shadows: bool = True

  @classmethod
  def look_at(cls, target, distance, yaw, pitch, fov=60., **kwargs):
    """The camera `distance` away from `target`, looking at it with `yaw` and `pitch` (degrees; see the module's text)."""
    y, p = math.radians(yaw), math.radians(pitch)
    if not abs(math.cos(p)) > 1e-9:
      raise ValueError('a pitch of +-90 degrees leaves right and up undefined')
    fwd = (-math.sin(y) * math.cos(p), math.cos(y) * math.cos(p), math.sin(p))
    right = (math.cos(y), math.sin(y), 0.)
    eye = tuple(float(t) - float(distance) * f for t, f in zip(target, fwd))
    return cls(eye=eye, fwd=fwd, right=right, up=_cross(right, fwd), fov=float(fov), **kwargs)

  @classmethod
  def reference(cls, config, **kwargs):
    """The reference's GUI view (env.py:275-281): target (sx / 2, sy / 2, 0), distance sqrt(sx^2 + sy^2 + sz^2) with
    (sx, sy, sz) = `Observer.size` (observer.py:355-357), yaw 45, pitch -45; vertical field of view 60."""
    sx = sy = config.overhead_res * config.pixel_size
    sz = config.max_z
    return cls.look_at((sx / 2, sy / 2, 0.), math.sqrt(sx * sx + sy * sy + sz * sz), 45., -45., **kwargs)

  def to_c(self, width, height):
    """The `srl_camera` of a `width` x `height` image: right scaled by tan(fov / 2) * width / height, up by tan(fov / 2)."""
    width, height = int(width), int(height)
    th = math.tan(math.radians(self.fov) / 2)
    tw = th * width / height if height > 0 else th
    c = CCamera()
    c.eye, c.fwd = _V3(*self.eye), _V3(*self.fwd)
    c.right, c.up = _V3(*(x * tw for x in self.right)), _V3(*(x * th for x in self.up))
    c.light = _V3(*_unit(self.light))
    c.ambient, c.diffuse = self.ambient, self.diffuse
    c.rock_rgb, c.sky_rgb = _V3(*self.rock_rgb), _V3(*self.sky_rgb)
    c.width, c.height, c.shadows = width, height, int(bool(self.shadows))
    return c
