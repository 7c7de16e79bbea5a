"""The training augmentations (augmentator.py, gen_utils.axis_rotation): Augmentator over Scaling, Rotation and Translation.

Host code: the generator hands `run` one (N, 3) or (N, 6) float32 numpy array per scan, before anything reaches the device.  What is
kept from the reference is what makes a run reproducible against it:
  * the draws come from numpy's GLOBAL generator, in the reference's order and number -- rand(1) for a scaling; rand(3) for a random
    axis (none for a fixed one), then rand(1) for the angle; rand(1, 3) for a translation -- so `np.random.seed(s)` gives the
    reference's transformation;
  * the arithmetic is the reference's: float64 factors and a float64 3x3 matrix against the float32 array, the float64 result stored
    back into the float32 array, in place.  Normals (columns 3..5) rotate with the points and are neither scaled nor translated.
What is refused: Rotation(..., "pca").  The reference's branch needs sklearn's PCA and calls `np.float`, which numpy 2 removed, so it
cannot run there either; a silent substitute would train on something else.

`from_config_string` evaluates the configuration's `aug_obj_str` ("aug.Augmentator([aug.Scaling([0.85, 1.15]), ...])",
generator.py:32) against a namespace that holds `aug` = this module and nothing else, builtins included."""
import sys

import numpy as np

AXES = ("fixed", "rand")


def _range(r, what):
    lo, hi = float(r[0]), float(r[1])
    if not hi > lo:
        raise ValueError(f"{what}: the range must be increasing, got [{r[0]}, {r[1]}]")
    return lo, hi


def _draw(shape, lo, hi):
    return np.random.rand(*shape) * (hi - lo) + lo


def axis_rotation(axis, angle):
    """gen_utils.axis_rotation: the float64 3x3 rotation by `angle` DEGREES about the unit vector `axis` (Rodrigues' formula)."""
    a = np.radians(float(np.asarray(angle).reshape(-1)[0]))
    x, y, z = (float(v) for v in axis)
    c, s = np.cos(a), np.sin(a)
    t = 1 - c
    return np.array([[c + x * x * t, x * y * t - z * s, x * z * t + y * s],
                     [y * x * t + z * s, c + y * y * t, y * z * t - x * s],
                     [z * x * t - y * s, z * y * t + x * s, c + z * z * t]], dtype=np.float64)


class Scaling:
    """xyz times one factor drawn uniformly from trans_range."""

    def __init__(self, trans_range):
        self.trans_range = trans_range
        self._lo, self._hi = _range(trans_range, "Scaling")

    def reload_val(self):
        self.trans_val = _draw((1,), self._lo, self._hi)

    def augment(self, vert_arr):
        vert_arr[:, :3] = vert_arr[:, :3] * self.trans_val
        return vert_arr


class Rotation:
    """xyz and, when present, the normals rotated by an angle in degrees drawn uniformly from angle_range, about z ("fixed") or about
    a drawn axis ("rand": rand(3) normalised, so always in the positive octant, as in the reference)."""

    def __init__(self, angle_range, angle_axis):
        if angle_axis == "pca":
            raise NotImplementedError("Rotation(..., 'pca') is not built: the reference's branch needs sklearn's PCA and calls np.float, which "
                                      "numpy 2 removed, so it does not run in the reference either; use 'fixed' or 'rand'")
        if angle_axis not in AXES:
            raise ValueError(f"Rotation: angle_axis must be one of {', '.join(AXES)}, got {angle_axis!r}")
        self.angle_range, self.angle_axis = angle_range, angle_axis
        self._lo, self._hi = _range(angle_range, "Rotation")

    def reload_val(self):
        if self.angle_axis == "rand":
            self.angle_axis_val = np.random.rand(3)
            self.angle_axis_val /= np.linalg.norm(self.angle_axis_val)
        else:
            self.angle_axis_val = np.array([0, 0, 1])
        self.rot_val = _draw((1,), self._lo, self._hi)

    def augment(self, vert_arr):
        rotation_mat = axis_rotation(self.angle_axis_val, self.rot_val)
        vert_arr[:, :3] = (rotation_mat @ vert_arr[:, :3].T).T
        if vert_arr.shape[1] == 6:
            vert_arr[:, 3:] = (rotation_mat @ vert_arr[:, 3:].T).T
        return vert_arr


class Translation:
    """xyz plus one vector whose three components are drawn uniformly from trans_range."""

    def __init__(self, trans_range):
        self.trans_range = trans_range
        self._lo, self._hi = _range(trans_range, "Translation")

    def reload_val(self):
        self.trans_val = _draw((1, 3), self._lo, self._hi)

    def augment(self, vert_arr):
        vert_arr[:, :3] = vert_arr[:, :3] + self.trans_val
        return vert_arr


class Augmentator:
    """reload_vals() draws every augmentation's parameters, in list order; run(mesh_arr) applies them in list order, in place."""

    def __init__(self, augmentation_list):
        self.augmentation_list = augmentation_list

    def run(self, mesh_arr):
        if not isinstance(mesh_arr, np.ndarray) or mesh_arr.ndim != 2 or mesh_arr.shape[1] not in (3, 6):
            raise ValueError(f"Augmentator.run takes a (N, 3) or (N, 6) numpy array, got {getattr(mesh_arr, 'shape', type(mesh_arr).__name__)}")
        for augmentation in self.augmentation_list:
            mesh_arr = augmentation.augment(mesh_arr)
        return mesh_arr

    def reload_vals(self):
        for augmentation in self.augmentation_list:
            augmentation.reload_val()


def from_config_string(aug_obj_str):
    """The object a configuration's `aug_obj_str` describes (None for None).  The string sees `aug` and no builtin: a configuration
    file is data here, not a program."""
    if aug_obj_str is None:
        return None
    return eval(aug_obj_str, {"__builtins__": {}, "aug": sys.modules[__name__]})  # noqa: S307
