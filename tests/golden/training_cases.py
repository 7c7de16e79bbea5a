"""The inputs of the training fixtures (make_golden_r17_training.py), shared by the generator and the tests, and the scripted stages that
stand in for tsegnet's two networks in the criterion case.  As in tsegnet_cases.py, everything scripted is built from exactly-rounded
float32 operations, so a CPU run of the reference and a GPU run of this package see the same values bit for bit."""
import numpy as np
import torch

import tsegnet_cases as TC

ROWS = 257                                   # points per array: odd, above one 256-wide block
AUG_SEEDS = (0, 1, 20221)
DEFAULT_CHAIN = "aug.Augmentator([aug.Scaling([0.85, 1.15]), aug.Rotation([-30,30], 'fixed'), aug.Translation([-0.2, 0.2])])"
SINGLES = {"scaling": "aug.Scaling([0.85, 1.15])", "rot_fixed": "aug.Rotation([-30,30], 'fixed')", "rot_rand": "aug.Rotation([-30,30], 'rand')",
           "translation": "aug.Translation([-0.2, 0.2])"}
PATIENTS = ("P01_upper", "P02_lower", "P03_upper")      # files <name>_sampled_points.npy; the split keeps P01 and P03
SPLIT = ("P01", "P03")
ITEM_SEED = 400                                         # np.random.seed(ITEM_SEED + k) in front of item k, k = the patient's position above
LR = {"lr": 1e-3, "min_lr": 1e-5, "full_steps": 40, "step_decay": 0.9, "steps": 45}
LOADERS = ((5, 2), (5, 15000000))                       # (loader length, schedueler_step)
VAL_LOSSES = (3.0, 2.0, 2.5)
LOSS_TERMS = (("dist_loss", 0.62109375, 1), ("chamf_loss", 1.2345678, 0.1), ("offset_1_loss", 3.0000002, 0.03))
LOSS_TERMS_2 = (("dist_loss", 0.25, 1), ("chamf_loss", 0.7654321, 0.1), ("offset_1_loss", 1e-3, 0.03))


def aug_arrays():
    """(257, 6) float32 rows: points of an arch-sized cloud, unit normals; and their first three columns."""
    rng = np.random.default_rng(1701)
    xyz = rng.uniform(-0.9, 0.9, (ROWS, 3))
    nrm = rng.standard_normal((ROWS, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    six = np.concatenate([xyz, nrm], 1).astype(np.float32)
    return six, np.ascontiguousarray(six[:, :3])


def patient_file(k):
    """The (257, 7) float64 array preprocess_data.py would have written for patient k: xyz, normal, label 0..16 (0 = gingiva)."""
    rng = np.random.default_rng(1710 + k)
    six = np.concatenate([rng.uniform(-0.9, 0.9, (ROWS, 3)), rng.standard_normal((ROWS, 3))], 1).astype(np.float32).astype(np.float64)
    lab = rng.integers(0, 17, (ROWS, 1)).astype(np.float64)
    return np.concatenate([six, lab], 1)


def criterion_case():
    """tsegnet_cases.module_case() with its one NaN distance replaced by 1.0: the proposal filter drops both, so the join and the crops
    are the r11 fixture's, and dist_loss is a number."""
    case = TC.module_case()
    case["dist"] = case["dist"].copy()
    case["dist"][0, 0, TC.FORCED[2]] = np.float32(1.0)
    return case


def train_seg(cropped):
    """The scripted segmentation stage of the criterion case, (T, C >= 3, k) -> (pd_1 (T, 2, k) probabilities, weight_1 (T, 1, k),
    pd_2 (T, 1, k), id_pred (T, 17)): functions of the xyz channels alone, column by column, of exactly-rounded operations."""
    xyz = cropped[:, :3, :]
    hi, lo = xyz.max(dim=2).values, xyz.min(dim=2).values
    c = (hi + lo) * 0.5
    d = xyz - c[:, :, None]
    dd = d * d
    r2 = (dd[:, 0, :] + dd[:, 1, :]) + dd[:, 2, :]
    m = TC.MASK_R2 - r2
    p = torch.clamp(m * 8.0 + 0.5, 0.0625, 0.9375)
    pd_1 = torch.stack([1.0 - p, p], 1)
    weight_1 = (d[:, 0, :] * 4.0)[:, None, :]
    pd_2 = (m * 40.0)[:, None, :]
    s = torch.floor((hi[:, 0] * 7.0 + hi[:, 1] * 3.0) * 16.0)
    j = torch.arange(17, dtype=cropped.dtype, device=cropped.device)
    id_pred = torch.remainder(s[:, None] + j * j, 7.0) * 0.5 - 1.0
    return pd_1, weight_1, pd_2, id_pred


class LearnedStage(torch.nn.Module):
    """A scripted stage with one parameter, `gain` = 1, that multiplies the floating outputs named in `scaled`: the scripted values
    unchanged, and a gradient path for a training step."""

    def __init__(self, fn, scaled):
        super().__init__()
        self.fn, self.scaled = fn, tuple(scaled)
        self.gain = torch.nn.Parameter(torch.ones(()))

    def forward(self, x):
        out = list(self.fn(x))
        for i in self.scaled:
            out[i] = out[i] * self.gain
        return tuple(out)
