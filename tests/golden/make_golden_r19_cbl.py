#!/usr/bin/env python3
"""Fixture of the contrastive-boundary criterion (tests/golden/reference_cpu_r19_cbl.npz), produced by running the REFERENCE's own
Python on CPU in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_r19_cbl.py [hand] [nets]

  hand   heads.ContrastHead.forward(None, target, stage_list) with default.yaml's configuration over the hand-made stage lists of
         cbl_cases.py, in float32, the latent features as autograd leaves.  `pointops.knnquery` (CUDA-only) is served by the CPU
         oracle, as make_golden_r4.py serves it.  Per case and stage: the loss, the stage labels and posmask as posmask_cnt saw and
         returned them, point_mask (0 < sum posmask < K - 1, checked against the number of rows the reference handed to its distance
         function) and the float32 autograd gradient with respect to the latents.  The reference alone runs every case: its stage-0
         `raise` is not reached.
  nets   cbl_point_transformer_module.get_model(...).forward([feats, target]) in eval mode with seeded weights at cbl_cases.NET_CASES,
         in float32 and in float64 on the same indices: the (block_num,) criterion and the number of contributing points per stage.

Both parts print the reference's own float32 error in the units of tests/cbl_ref.py; cbl_cases.py's MEASURED / NET_MEASURED and the
bounds derived from them are copied from that output."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TGN_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cbl_cases as CC  # noqa: E402
import cbl_ref  # noqa: E402
from make_golden import load_reference  # noqa: E402
from make_golden_r3 import cpu_as_cuda  # noqa: E402
from make_golden_r4 import _serve_pointops  # noqa: E402
from oracle import cpu as O  # noqa: E402
from seeded import seeded_fill  # noqa: E402


class Recorder:
    """What ContrastHead's own helpers saw, per call (= per stage): posmask_cnt's labels and result, dist_l2's row count."""

    def __init__(self, H):
        self.H, self.stages = H, []
        self.keep = (H.ContrastHead.posmask_cnt, H.ContrastHead.dist_l2)

    def __enter__(self):
        # (ContrastHead binds dist_l2 when it is constructed: build the head or the network inside the `with`)
        keep_pos, keep_dist, rec = self.keep[0], self.keep[1], self

        def posmask_cnt(head, labels, neighbor_label):
            mask = keep_pos(head, labels, neighbor_label)
            rec.stages.append(dict(labels=torch.argmax(labels, -1).numpy().copy(), posmask=mask.numpy().copy(), rows=0))
            return mask

        def dist_l2(head, features, neighbor_feature):
            rec.stages[-1]["rows"] = int(features.shape[0])
            return keep_dist(head, features, neighbor_feature)
        self.H.ContrastHead.posmask_cnt, self.H.ContrastHead.dist_l2 = posmask_cnt, dist_l2
        return self

    def __exit__(self, *exc):
        self.H.ContrastHead.posmask_cnt, self.H.ContrastHead.dist_l2 = self.keep


def criterion_config(M, ncls, nsample, stride):
    """What get_model hands to ContrastHead (cbl_point_transformer_module.py:220-235, :61-62)."""
    from models.modules.cbl_point_transformer.util import config as cfgmod
    cfg = cfgmod.CfgNode(cfgmod.load_cfg_from_cfg_file(os.path.join(os.path.dirname(M.__file__), "default.yaml")), default="")
    cfg["base_fdim"], cfg["nstride"], cfg["nsample"], cfg["stride"] = 32, list(stride), list(nsample), list(stride)
    cfg.num_layers, cfg.num_classes = len(nsample), ncls
    return cfg


def hand_part(M, H, out):
    worst_loss = worst_grad = 0.0
    for name in CC.HAND_CASES:
        case = CC.build(name)
        cfg = criterion_config(M, case["ncls"], case["nsample"], case["stride"])
        leaves = [torch.from_numpy(f).clone().requires_grad_() for f in case["f"]]
        stage_list = {"up": [{"p_out": torch.from_numpy(p), "latent": x, "offset": torch.from_numpy(o)}
                             for p, x, o in zip(case["p"], leaves, case["o"])]}
        with Recorder(H) as rec:
            head = H.ContrastHead(cfg.contrast, cfg)
            losses = head(None, torch.from_numpy(case["target"]), stage_list)          # the stage-0 `raise` would end the run here
        exact = cbl_ref.all_stages(O.knnquery, case)
        case_loss = case_grad = 0.0
        for i, (loss, leaf, seen, ex) in enumerate(zip(losses, leaves, rec.stages, exact)):
            K1 = case["nsample"][i] - 1
            npos = seen["posmask"].sum(1)
            point_mask = (npos > 0) & (npos < K1)
            assert int(point_mask.sum()) == seen["rows"], (name, i, int(point_mask.sum()), seen["rows"])
            grad = np.zeros_like(case["f"][i])
            if loss.requires_grad:
                grad = torch.autograd.grad(loss, leaf)[0].numpy()
            g64, gscale = ex["grad"]()
            lu = cbl_ref.loss_units(float(loss.detach()), float(ex["loss"].detach()), ex["loss_scale"])
            gu = cbl_ref.grad_units(grad, g64, gscale)
            case_loss, case_grad = max(case_loss, lu), max(case_grad, gu)
            print(f"  {name} stage {i}: loss {float(loss.detach()):.9g} (float64 {float(ex['loss'].detach()):.12g}), {seen['rows']} of {len(npos)} points "
                  f"contribute, no positive {int((npos == 0).sum())}, all positive {int((npos == K1).sum())}, vote ties {int(ex['tie'].sum())}; "
                  f"reference fp32 error: loss {lu:.2f}, gradient {gu:.2f} units")
            out[f"{name}_loss_{i}"] = np.float32(float(loss.detach()))
            out[f"{name}_labels_{i}"] = seen["labels"].astype(np.int16)
            out[f"{name}_posmask_{i}"] = seen["posmask"]
            out[f"{name}_point_mask_{i}"] = point_mask
            out[f"{name}_grad_{i}"] = grad.astype(np.float32)
        # every rule is reached, by the reference alone
        s0 = rec.stages[0]["posmask"].sum(1)
        K1 = case["nsample"][0] - 1
        assert (s0 == 0).any() and (s0 == K1).any() and ((s0 > 0) & (s0 < K1)).any(), "stage 0: no positive, all positive, mixed"
        assert rec.stages[0]["posmask"][case["planted"]].sum() == 0, "the planted point has no positive neighbour"
        if name == "blobs4":
            assert rec.stages[2]["rows"] == 0 and float(losses[2]) == 0.0, "stage 2 has no mixed point"
            assert exact[2]["tie"][case["tie"]] and rec.stages[2]["labels"][case["tie"]] == 1, "the 2 : 2 vote goes to the lowest label"
            assert set(rec.stages[2]["labels"][:6]) == {1} and set(rec.stages[2]["labels"][6:]) == {2}
        else:
            assert rec.stages[2]["rows"] > 0, "stage 2 is mixed over padded lists"
        assert all(r["rows"] > 0 for r in rec.stages[:2])
        print(f"  {name}: reference fp32 error, largest over the stages: loss {case_loss:.4f}, gradient {case_grad:.4f} units")
        worst_loss, worst_grad = max(worst_loss, case_loss), max(worst_grad, case_grad)
    print(f"  hand cases: MEASURED loss {worst_loss:.2f} -> bound {CC._pow2_at_least(2 * worst_loss):g}; gradient {worst_grad:.2f} -> bound "
          f"{CC._pow2_at_least(2 * worst_grad):g}")


def nets_part(M, H, RP, out):
    keep = _serve_pointops(RP)
    worst = 0.0
    try:
        for name, (arch, k, B, N, wseed, _) in CC.NET_CASES.items():
            feats, labels = CC.net_inputs(name)
            res = {}
            for tag, ftype, dt in (("32", torch.FloatTensor, torch.float32), ("64", torch.DoubleTensor, torch.float64)):
                with Recorder(H) as rec, torch.no_grad(), cpu_as_cuda(ftype):
                    net = M.get_model(k=k, **arch).eval()
                    seeded_fill(net, wseed)
                    y = net.to(dt)([torch.from_numpy(feats).to(dt), torch.from_numpy(labels)])
                assert len(y) == 5 and (y[2] is None) == (B > 1)
                res[tag] = (y[0].double().numpy(), np.array([s["rows"] for s in rec.stages]))
            (l32, c32), (l64, c64) = res["32"], res["64"]
            assert np.array_equal(c32, c64) and len(c32) == arch["block_num"], "the masks depend on geometry and labels only"
            # units: float32 epsilon times 0.1 * (1 + per-point loss) averaged = eps * (0.1 + loss), the loss scale of cbl_ref
            units = np.abs(l32 - l64) / (cbl_ref.EPS32 * (cbl_ref.WEIGHT + np.abs(l64)))
            print(f"  {name}: cbl {np.array2string(l64, precision=6)} counts {c64.tolist()}; reference fp32 network against float64: "
                  f"{np.array2string(units, precision=1)} units, largest {units.max():.4f}")
            worst = max(worst, float(units.max()))
            out[f"net_{name}_loss_32"], out[f"net_{name}_loss_64"], out[f"net_{name}_counts"] = l32.astype(np.float32), l64, c64.astype(np.int32)
    finally:
        RP.furthestsampling, RP.knnquery = keep
    print(f"  network cases: NET_MEASURED largest {worst:.1f} units -> bound {CC._pow2_at_least(2 * worst):g}")


def main():
    torch.set_num_threads(8)
    parts = sys.argv[1:] or ["hand", "nets"]
    path = os.path.join(HERE, "reference_cpu_r19_cbl.npz")
    out = dict(np.load(path)) if os.path.exists(path) else {}
    load_reference()
    if REFERENCE not in sys.path:
        sys.path.append(REFERENCE)
    import models.modules.cbl_point_transformer.cbl_point_transformer_module as M
    import models.modules.cbl_point_transformer.blocks as RB
    import models.modules.cbl_point_transformer.heads as H
    import models.modules.cbl_point_transformer.basic_operators as BO
    RP = RB.pointops
    assert all(m.__file__.startswith(REFERENCE) for m in (M, H, BO, RP))
    assert H.pointops is RP and BO.pointops is RP
    if "hand" in parts:
        keep = _serve_pointops(RP)
        try:
            hand_part(M, H, out)
        finally:
            RP.furthestsampling, RP.knnquery = keep
    if "nets" in parts:
        nets_part(M, H, RP, out)
    np.savez_compressed(path, **out)
    print(f"wrote tests/golden/reference_cpu_r19_cbl.npz ({os.path.getsize(path) / 1e3:.1f} kB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
