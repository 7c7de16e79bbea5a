"""GPU: every function of toothgroupnetwork_amd/tgnet.py that reaches the library, called with strided, offset, expanded, float64 /
float16 / bfloat16 and int32 operands, in the manner of tests/test_gpu_operator_forms.py (whose helpers and values -- multiples of 1/16,
exact in every float dtype -- this imports): each form gives the packed call's bits, or raises naming the argument."""
import numpy as np
import pytest
import torch

import operator_forms as T

pytestmark = pytest.mark.gpu


def _same(got, want, what, follows=False):
    got, want = T._tensors(got), T._tensors(want)
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        if follows and g.is_floating_point():                   # rows selected from the argument come back in the argument's dtype
            g, w = g.double(), w.double()
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w.cpu()), what


def _sweep(call, build, floats, ints, expand=(), names=None, follows=False):
    """call(**build()) with every form of every tensor argument: the baseline's outputs, or a raise that names the argument"""
    names = names or {}
    want = call(**build())
    probes = 0
    for arg in floats + ints:
        base = build()
        forms = T.float_forms_of({"expand": expand}, arg, base[arg]) if arg in floats else T.index_forms_of(base[arg])
        for form, probe in forms:
            ref = want if form != "expanded" else call(**dict(build(), **{arg: probe.contiguous()}))
            try:
                got = call(**dict(build(), **{arg: probe}))
            except T.RAISES as e:
                assert names.get(arg, arg) in str(e), f"{arg}:{form} raised without naming the argument: {e}"
            else:
                _same(got, ref, f"{arg}:{form}", follows)
            probes += 1
    assert probes >= 2 * len(floats + ints)
    _same(call(**build()), want, "the baseline after the probes")


def test_crop_vote_forms(dev):
    from toothgroupnetwork_amd import tgnet
    g = T.gen_for("tgnet.crop_vote")

    def build():
        g.manual_seed(1)
        idx = torch.stack([torch.randperm(40, generator=g)[:16] for _ in range(3)])
        return dict(sem_2=T.q16(g, 3, 2, 16).to(dev), idx=idx.to(dev))
    _sweep(lambda sem_2, idx: tgnet.crop_vote(sem_2, idx, 40), build, ["sem_2"], ["idx"], names={"idx": "nn_crop_indexes"})


def test_boundary_flags_forms(dev):
    from toothgroupnetwork_amd import tgnet

    def build():
        g = T.gen_for("tgnet.boundary_flags")
        sampled = T.q16(g, 300, 3)
        return dict(dense=T.q16(g, 200, 3).double().to(dev), sampled=sampled.double().to(dev),
                    labels=(sampled[:, 0] > 0).long().to(dev) + (sampled[:, 1] > 1).long().to(dev))
    _sweep(lambda dense, sampled, labels: tgnet.boundary_flags(dense, sampled, labels), build, ["dense", "sampled"], ["labels"],
           expand=("dense",), names={"dense": "dense_xyz", "sampled": "sampled_xyz", "labels": "point_labels"})
    a = build()
    _same(tgnet.boundary_flags(a["dense"], a["sampled"], a["labels"].double()), tgnet.boundary_flags(**{"dense_xyz": a["dense"],
          "sampled_xyz": a["sampled"], "point_labels": a["labels"]}), "labels kept in a float64 column, as the reference keeps them")
    with pytest.raises(TypeError, match="dense_xyz"):
        tgnet.boundary_flags(a["dense"].long(), a["sampled"], a["labels"])


def test_boundary_resample_forms(dev):
    from toothgroupnetwork_amd import tgnet
    info = {"bdl_ratio": 0.7, "num_of_bdl_points": 64, "num_of_all_points": 256}

    def build():
        g = T.gen_for("tgnet.boundary_resample")
        grid = torch.stack(torch.meshgrid(torch.arange(24.0), torch.arange(24.0), indexing="ij"), -1).reshape(-1, 2) / 4 - 3
        dense = torch.cat([grid, torch.zeros(576, 1), T.q16(g, 576, 3)], 1)[torch.randperm(576, generator=g)]
        return dict(dense=dense.double().to(dev), sampled=dense[::2].double().to(dev), labels=(dense[::2, 0] > 0).long().to(dev))

    def call(dense, sampled, labels):
        np.random.seed(3)
        return tgnet.boundary_resample(dense, sampled, labels, info, carry=(torch.arange(576, device=dev),))
    _sweep(call, build, ["dense", "sampled"], ["labels"], names={"dense": "dense", "sampled": "sampled", "labels": "point_labels"},
           follows=True)


def test_kmeans_forms(dev):
    from toothgroupnetwork_amd import tgnet

    def build():
        pts, g = T._blobs("tgnet.kmeans", 300, 3)
        return dict(points=pts.to(dev), init=(pts[:4] * 0.5).double().to(dev))
    _sweep(lambda points, init: tgnet.kmeans(points, init), build, ["points", "init"], [], expand=("points",),
           names={"init": "init_centres"})
    a = build()
    labels, cent = tgnet.kmeans(a["points"], a["init"])
    assert labels.dtype == torch.int64 and cent.dtype == torch.float64 and len(torch.unique(labels)) >= 3
    with pytest.raises(TypeError, match="init_centres"):
        tgnet.kmeans(a["points"], a["init"].long())


def _pass_build(dev):
    """first_instances / second_instances on operator_forms' clustering case: the moved points ARE the points (offset 0), one crop
    holds every point and masks the gingiva out"""
    a = T._gcl_build(dev)
    moved, labels = a["moved_points"], a["labels"]
    n = moved.shape[0]
    g = T.gen_for("tgnet.passes")
    feats = torch.cat([moved.t(), torch.zeros(3, n, device=dev)])[None].contiguous()
    fg = (labels != 0).float()
    return dict(feats=feats, sem_1=T.q16(g, 1, 10, n).to(dev), offset_1=torch.zeros(1, 3, n, device=dev),
                sem_2=torch.stack([torch.full_like(fg, 0.5), fg])[None].contiguous(), idx=torch.arange(n, device=dev)[None].contiguous(),
                labels=(torch.arange(n, device=dev) % 3 * (labels != 0)).contiguous())


def test_first_instances_forms(dev):
    from toothgroupnetwork_amd import tgnet

    def call(feats, sem_1, offset_1, sem_2, idx, labels):
        out = tgnet.first_instances(feats, {"sem_1": sem_1, "offset_1": offset_1, "sem_2": sem_2, "nn_crop_indexes": [idx]})
        return [out[k] for k in ("xyz", "sem", "mask", "moved", "ins")]
    _sweep(call, lambda: _pass_build(dev), ["feats", "sem_1", "offset_1", "sem_2"], ["idx"], names={"idx": "nn_crop_indexes"})
    ins = call(**_pass_build(dev))[4]
    assert len(torch.unique(ins)) == 7, "background and the six clusters of operator_forms' case (three blobs of two grid points each)"


def test_second_instances_forms(dev):
    from toothgroupnetwork_amd import tgnet

    def call(feats, sem_1, offset_1, sem_2, idx, labels):
        out = tgnet.second_instances(feats, labels, {"offset_1": offset_1, "sem_2": sem_2, "nn_crop_indexes": [idx]})
        return [out[k] for k in ("xyz", "mask", "moved", "ins", "centres")]
    _sweep(call, lambda: _pass_build(dev), ["feats", "offset_1", "sem_2"], ["idx", "labels"], names={"idx": "nn_crop_indexes"})
    ins = call(**_pass_build(dev))[3]
    assert len(torch.unique(ins)) == 3, "k = len(unique(labels)) - 1 = 2 clusters and the background"


def test_merge_boundary_forms(dev):
    from toothgroupnetwork_amd import tgnet

    def build():
        g = T.gen_for("tgnet.merge_boundary")
        first = T.q16(g, 200, 3)
        return dict(first_xyz=first.double().to(dev), first_ins=(first[:, 0] > 0).long().to(dev) * 2, bdl_xyz=T.q16(g, 90, 3).double().to(dev),
                    bdl_ins=(torch.arange(90) % 4).to(dev))

    def call(first_xyz, first_ins, bdl_xyz, bdl_ins):
        return [torch.from_numpy(v) for v in tgnet.merge_boundary(first_xyz, first_ins, first_ins * 3, bdl_xyz, bdl_ins)]
    _sweep(call, build, ["first_xyz", "bdl_xyz"], ["first_ins", "bdl_ins"])
