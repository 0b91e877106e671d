"""dynamics.pth compatibility against the reference's checkpoint layout.  The reference's file is 13 MB
(3.27 M fp32 parameters incl. the saved_* copies), too large to commit as a fixture, so tests/golden/g19_dynamics_pth.json
records what the reference's `MOBODYEnsembleDynamics.save` (mobody_dynamics.py:1158-1161) writes for the G2 walker model:
the state_dict's keys in order with shape and dtype, its `_metadata`, the constant buffers and the scaler files.  This test

  (1) rebuilds a file of exactly that layout (G2 weights, seeded values in the tensors the G2 fixture does not pin) and
      loads it through the mirror's `.load()` (torch.load(weights_only=True)) -> every tensor of the mirror's state_dict
      equals the file's, key for key (saved_weight/saved_bias, za_de_*, max/min_logvar(_latent), elites);
  (2) has the mirror `.save()` it again and reads THAT the way the reference's `.load()` does (torch.load +
      strict load_state_dict; load_scaler's np.load(allow_pickle=True) + torch.FloatTensor of the scaler files) -> same
      files, same keys, shapes and dtypes as the reference writes, every tensor as loaded in (1), and scaler files that
      load_scaler can convert (the reference's own pickled None cannot be: torch.FloatTensor raises) holding the
      identity scaling (mu = 0, std = 1) that load_scaler then sets anyway.

Needs no GPU."""
import collections
import json
import os

import numpy as np
import torch

import golden_util as gu


def _layout():
    with open(os.path.join(gu.GOLDEN, "g19_dynamics_pth.json")) as f:
        return json.load(f)


def _reference_layout_file(d, lay, p):
    """dynamics.pth + mu.npy + std.npy as the reference's save writes them, with the G2 weights."""
    rng = np.random.default_rng(19)
    sd = collections.OrderedDict()
    for e in lay["keys"]:
        k, shape, dtype = e["name"], tuple(e["shape"]), getattr(torch, e["dtype"])
        if k in lay["constants"]:
            v = torch.tensor(lay["constants"][k], dtype=dtype)
        elif k in p:
            v = torch.from_numpy(p[k].copy())
        else:                                            # saved_* copies and the za_de_* decoders: not pinned by G2
            v = torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * 0.1)
        assert tuple(v.shape) == shape and v.dtype == dtype, k
        sd[k] = v
    sd._metadata = collections.OrderedDict((m, {"version": 1}) for m in lay["metadata"])
    torch.save(sd, os.path.join(d, "dynamics.pth"))
    for f, s in lay["scaler"].items():
        assert s["dtype"] == "object" and s["value"] == "None"
        np.save(os.path.join(d, f), None)
    return sd


def test_dynamics_checkpoint_round_trip_with_the_reference(tmp_path):
    g = gu.load("g234_dynamics_walker")
    S, A = int(g["S"]), int(g["A"])
    lay = _layout()
    assert (lay["S"], lay["A"]) == (S, A)
    p = gu.dyn_params_for(g)

    d1 = tmp_path / "ref_written"; d1.mkdir()
    want = _reference_layout_file(str(d1), lay, p)
    assert sorted(os.listdir(d1)) == lay["files"] == ["dynamics.pth", "mu.npy", "std.npy"]

    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    from mobody_amd.algo.mb_utils.terminal_funs import get_termination_fn
    mcfg = gu.policy_cfg(S, A)
    mm = MOBODYModule(S, A, 256, 7, 5, device="cpu", config=mcfg)
    md = MOBODYEnsembleDynamics(mcfg, mm, None, None, get_termination_fn("walker2d-medium-v2"), penalty_coef=0.1)
    md.load(str(d1))                                                       # (1) reference layout -> mirror
    got = mm.state_dict()
    assert sorted(want) == sorted(got)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k].cpu(), want[k]), k
    assert [int(x) for x in mm.elites.tolist()] == [6, 2, 3, 5, 4]
    assert (md.obs_scaler.mu, md.obs_scaler.std) == (0, 1)                   # load_scaler's end state (:153-154)

    d2 = tmp_path / "mirror_written"; d2.mkdir()
    md.save(str(d2))                                                       # (2) mirror-written -> reference's load
    assert sorted(os.listdir(d2)) == lay["files"]
    sd = torch.load(str(d2 / "dynamics.pth"), map_location="cpu", weights_only=True)
    # strict load_state_dict of the reference's module: no missing or unexpected key, every shape as the module's
    assert sorted(sd) == sorted(e["name"] for e in lay["keys"])
    for e in lay["keys"]:
        k = e["name"]
        assert tuple(sd[k].shape) == tuple(e["shape"]) and sd[k].dtype == getattr(torch, e["dtype"]), k
        assert torch.equal(sd[k], want[k]), k
    for f, ident in (("mu.npy", 0.0), ("std.npy", 1.0)):                   # load_scaler (:144-154)
        x = torch.FloatTensor(np.load(str(d2 / f), allow_pickle=True))
        assert x.dtype == torch.float32 and x.numel() > 0 and bool((x == ident).all()), f
        ref = np.load(str(d1 / f), allow_pickle=True)                      # what the reference itself writes (g19)
        assert str(ref.dtype) == lay["scaler"][f]["dtype"] and repr(ref.item()) == lay["scaler"][f]["value"], f
