"""adaptive_stereo.consistency on the GPU: predict_disparity_leftright against the oracle (both views inside
tests/test_gpu_end_to_end.py's EPE_BAR), BothViewInference against the restatement applied to its own disparities (given the maps
every decision is exact: bit for bit, no pixel left out), eager against a graph replay, the cloud gated by valid_l against
pointcloud_ref, and evaluate_model.py --lr_check.  Networks and inputs as test_gpu_matches_oracle_on_fresh_inputs builds them."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import confidence_ref as cr
import lr_consistency_ref as lr
import pointcloud_ref as pr
from conftest import parity_note
from dataset_fixture import make_tree
from test_gpu_end_to_end import EPE_BAR, build
from adaptive_stereo import consistency as cons
from adaptive_stereo.pointcloud import DepthProjector, StereoCamera
from adaptive_stereo.utils import synthetic as syn
from guarded_buffers import DEV, same_bits
from oracle import stereo_oracle as orc

B, H, W, K, MAXDISP = 2, 83, 150, 3, 100


def _np_bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def world():
  """the networks in eval mode, two different batches of pairs on the device, and the library's both-view outputs of the first"""
  fnet, snet = build(dict(k=K, s=0, maxdisp=MAXDISP, gain=200.0))
  fnet.eval(); snet.eval()
  pairs = [syn.stereo_pair(B, H, W, seed=seed, disparities=(3.0, 9.0, 14.0)[:B]) for seed in (7, 8)]
  dev_pairs = [(l.to(DEV).contiguous(), r.to(DEV).contiguous()) for l, r in pairs]
  out = cons.predict_disparity_leftright(fnet, snet, dev_pairs[0][0], dev_pairs[0][1], output_cost_volume=True)
  return dict(fnet=fnet, snet=snet, pairs=pairs, dev_pairs=dev_pairs, out=out)


def check_against_restatement(disp_l, disp_r, chk, filled, tol=(1.0, 0.0)):
  want = lr.lr_check(disp_l.cpu().numpy(), disp_r.cpu().numpy(), *tol)
  for k in chk._fields:
    assert same_bits(getattr(chk, k), want[k]), k
  assert same_bits(filled, lr.lr_fill(disp_l.cpu().numpy(), want["code_l"]))
  return want


def test_both_views_match_the_oracle(world):
  left, right = world["pairs"][0]
  fsd = {n: t.detach().cpu().clone() for n, t in world["fnet"].state_dict().items()}
  ssd = {n: t.detach().cpu().clone() for n, t in world["snet"].state_dict().items()}
  ref_l, _ = orc.forward_only(fsd, ssd, left, right, K, 0, MAXDISP)
  ref_x, _ = orc.forward_only(fsd, ssd, torch.flip(right, (-1,)), torch.flip(left, (-1,)), K, 0, MAXDISP)    # the mirrored, swapped pair
  out = world["out"]
  epe_l = float((out["pred_disp_l/0"].cpu() - ref_l["pred_disp_l/0"]).abs().mean())
  epe_r = float((out["pred_disp_r/0"].cpu() - torch.flip(ref_x["pred_disp_l/0"], (-1,))).abs().mean())
  parity_note("both_view_eval", epe_l=epe_l, epe_r=epe_r)
  assert epe_l <= EPE_BAR and epe_r <= EPE_BAR, (epe_l, epe_r)
  # the reference's key set, every _x key once as _l and once as _r
  with torch.no_grad():
    ld = world["dev_pairs"][0][0]
    feats = world["fnet"](ld)
    keys_x = set(world["snet"](ld, feats, feats, "x", output_cost_volume=True).keys())
  assert keys_x == {"cost_volume_x/%d" % K, "pred_disp_x/%d" % K, "pred_disp_x/0"}
  assert set(out.keys()) == {k.replace("_x", "_l") for k in keys_x} | {k.replace("_x", "_r") for k in keys_x}
  for k, v in out.items():
    assert v.shape[0] == B and v.is_contiguous() and not v.requires_grad, k
  without = cons.predict_disparity_leftright(world["fnet"], world["snet"], *world["dev_pairs"][0])
  assert set(without.keys()) == {"pred_disp_l/%d" % K, "pred_disp_r/%d" % K, "pred_disp_l/0", "pred_disp_r/0"}
  assert torch.equal(without["pred_disp_r/0"], out["pred_disp_r/0"])


def test_training_mode_raises(world):
  fnet, snet = world["fnet"], world["snet"]
  left, right = world["dev_pairs"][0]
  for net in (fnet, snet):
    net.train()
    try:
      with pytest.raises(RuntimeError, match="inference only"):
        cons.predict_disparity_leftright(fnet, snet, left, right)
      with pytest.raises(RuntimeError, match="inference only"):
        cons.BothViewInference(fnet, snet, H, W, batch=B)(left, right)
    finally:
      net.eval()
  import adapt
  from adaptive_stereo.control import State
  via_adapt = adapt.predict_disparity_leftright(fnet, snet, left, right, State.VALIDATION, None)
  assert set(via_adapt.keys()) == set(world["out"].keys())
  assert torch.equal(via_adapt["pred_disp_r/0"], world["out"]["pred_disp_r/0"])
  with pytest.raises(NotImplementedError, match="leftright_consistency"):
    adapt.predict_disparity_leftright(fnet, snet, left, right, State.IN_PROGRESS, None)


def test_both_view_inference_eager_and_replayed(world):
  fnet, snet = world["fnet"], world["snet"]
  (l0, r0), (l1, r1) = world["dev_pairs"]
  both = cons.BothViewInference(fnet, snet, H, W, batch=B)
  disp_l, disp_r, chk, filled = both(l0, r0)
  torch.cuda.synchronize()
  assert torch.equal(disp_l, world["out"]["pred_disp_l/0"]) and torch.equal(disp_r, world["out"]["pred_disp_r/0"])
  want = check_against_restatement(disp_l, disp_r, chk, filled)
  disp_l = disp_l.clone()
  assert len(np.unique(want["code_l"])) >= 3, "the scene exercises the check"        # consistent, rejected, out of view
  assert np.allclose(both.lrc.fractions().sum(axis=2), 1.0)
  e = both(l1, r1)
  eager = [t.clone() for t in (e[0], e[1]) + tuple(e[2]) + (e[3],)]                  # the buffers are overwritten by the next call
  assert not torch.equal(eager[0], disp_l)                                           # a different pair

  outer, side, x = torch.cuda.CUDAGraph(), torch.cuda.Stream(), torch.zeros(4, device=DEV)
  torch.cuda.synchronize()
  with torch.cuda.graph(outer, stream=side, capture_error_mode="thread_local"):
    x.add_(1.0)
    with pytest.raises(RuntimeError, match="already being captured"):               # refused before anything is issued
      both.capture()
  both.capture(l0, r0)
  r_disp_l, r_disp_r, r_chk, r_filled = both(l1, r1)                                 # a copy into the static inputs + one replay
  torch.cuda.synchronize()
  replayed = [r_disp_l, r_disp_r] + list(r_chk) + [r_filled]
  assert len(replayed) == len(eager)
  for i, (a, b) in enumerate(zip(replayed, eager)):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "output %d differs between replay and eager" % i
  check_against_restatement(r_disp_l, r_disp_r, r_chk, r_filled)
  sl, sr = both.inputs()
  assert torch.equal(sl, l1) and torch.equal(sr, r1)


def test_cloud_gated_by_the_check(world):
  left = world["dev_pairs"][0][0]
  disp_l, disp_r = world["out"]["pred_disp_l/0"].contiguous(), world["out"]["pred_disp_r/0"]
  lrc = cons.LeftRightConsistency(H, W, batch=B, device=DEV)
  chk = lrc.check(disp_l, disp_r)
  cam = StereoCamera(721.5, 721.5 * 1.03, 0.37 * W + 0.3, 0.45 * H + 0.7, 0.54)
  proj = DepthProjector(H, W, cam, batch=B, pyramid_scale=0, device=DEV)
  cloud = proj.voxel_cloud(disp_l, left, confidence=chk.valid_l, conf_min=1.0)
  level = proj.confidence_level.cpu().numpy()                                       # the library's own map at the projector's level
  assert np.array_equal(_np_bits(level), _np_bits(chk.valid_l.cpu().numpy())), "valid_l reaches the gate unchanged"
  host_disp, host_left = disp_l.cpu().numpy(), left.cpu().numpy()
  consts = pr.camera_constants(cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline, 0)
  p = pr.points(host_disp, consts, 0)
  q, rejected = cr.gate(p, level[:, 0], 1.0)                                        # valid &= conf >= conf_min
  assert cloud.rejected.tolist() == rejected.tolist() and all(0 < r for r in rejected)
  got = cloud.trim()
  for b in range(B):
    ref = pr.voxel_cloud(q, b, 0.15, pr.colour_bytes(host_left, 0))
    g = got[b]
    assert int(cloud.n[b]) == ref["n"] and g["dropped"] == ref["dropped"]
    vox, cnt, rec = pr.sort_cloud(g["voxel"].cpu().numpy(), g["count"].cpu().numpy(), g["records"].cpu().numpy())
    assert np.array_equal(vox, ref["voxel"]) and np.array_equal(cnt, ref["count"])
    assert np.array_equal(rec[:, :3], _np_bits(ref["xyz"])) and np.array_equal(rec[:, 3].view(np.uint32), ref["rgb"])


def test_evaluate_model_lr_check_saves_the_extra_outputs(tmp_path):
  import evaluate_model as E
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  k, h, w, n = 3, 64, 96, 3
  data, splits = make_tree(str(tmp_path), "KittiStereo2015", n=n, H0=70, W0=110, seed=3)
  weights = str(tmp_path / "weights")
  os.makedirs(weights)
  fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0)
  torch.save(syn.synthetic_state_dict(fnet.state_dict(), seed=123), os.path.join(weights, "feature_net.pth"))
  torch.save(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=5.0), os.path.join(weights, "stereo_net.pth"))
  args = ["--dataset_path", data, "--dataset_name", "KittiStereo2015", "--split", "tiny", "--subsplit", "train",
          "--splits_path", splits, "--load_weights_folder", weights, "--stereonet_k", str(k), "--batch_size", "2",
          "--height", str(h), "--width", str(w), "--num_workers", "0"]
  E.main(E.make_parser().parse_args(["--mode", "save", "--lr_check"] + args))
  folder = os.path.join(weights, "outputs", "tiny")
  extra = {"pred_disp_r_0": torch.float32, "lr_code_l_0": torch.uint8, "pred_disp_l_filled_0": torch.float32}
  assert set(extra) | {"pred_disp_l_0"} <= set(os.listdir(folder))
  for name, dtype in extra.items():
    assert sorted(os.listdir(os.path.join(folder, name))) == ["%04d.pt" % i for i in range(n)], name
    for i in range(n):
      t = torch.load(os.path.join(folder, name, "%04d.pt" % i))
      assert tuple(t.shape) == (1, h, w) and t.dtype == dtype and not t.is_cuda, (name, i, t.shape, t.dtype)
  E.main(E.make_parser().parse_args(["--mode", "eval", "--lr_check"] + args))          # runs; its numbers are the kernels' above
  assert not E.make_parser().parse_args(["--mode", "save"] + args).lr_check            # default off
