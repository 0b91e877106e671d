"""csrc/pretrain.hip against fp64, ONE LOSS TERM AT A TIME (tests/pretrain_terms.py; the rule's teeth: test_pretrain_terms.py).

mobody_pretrain_grads takes the three coefficients that separate the terms, so each tensor is compared at the scale of the
isolated term: the chain rule through std_e(mean6) (k_pre_fake_bwd), the KL part of dz3enc (k_pre_latent_bwd), the source
domain's 0.01, the action-encoder gradient (phase H + k_pre_za_reduce, which no fp64 test looked at).  The geometries walk
every remainder of k_pre_za_reduce's unrolled chunk loop, A > S and Np3 > 2S.  Rule, both MFMA modes:
    max|hip - ref64| <= 3 max|ref32 - ref64| + 1e-6 max|ref64| + 1e-12   per tensor,
a tensor the term does not reach is exactly zero, losses at rtol 2e-5 / atol 1e-7.

Every call runs on a workspace filled with NaN and a gradient blob filled with a NaN of a payload of its own: whatever a kernel
reads without having written it, or leaves unwritten, shows.  The unused action encoder's region keeps the payload ("left
untouched", include/mobody_hip.h); layout padding inside the written regions is exactly 0.

The fused single-GPU step (mobody_pretrain_update) equals mobody_pretrain_grads + mobody_pretrain_adam bit for bit when both get
the same explicit noise and host step counts: both reduce through the same element functions.

The measured err / bound of every (geometry, term, domain, mode, tensor) is kept in profiles/pretrain_terms_bounds.json (set
MOBODY_PRETRAIN_TERMS_JSON=<path> to rewrite it).
"""
import json
import os

import numpy as np
import pytest
import torch

import pretrain_terms as PT

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                       # a quiet NaN no arithmetic produces
RATIOS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def bounds_file():
    yield
    path = os.environ.get("MOBODY_PRETRAIN_TERMS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"what": "|hip - fp64| / (3 |fp32 - fp64| + 1e-6 |fp64|) per tensor, tests/test_hip_pretrain_terms.py",
                       "cases": RATIOS}, f, indent=0, sort_keys=True)


def sentinel_blob(n, dev):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


class Case:
    """Device copies of a case's inputs, a NaN workspace and the blob's map: which floats are parameters, which padding."""

    def __init__(self, S, A, b, term, mode, dev):
        from mobody_amd import _lib, ops, packing
        self.ops, self.packing, self.S, self.A, self.b, self.term, self.mode, self.dev = ops, packing, S, A, b, term, mode, dev
        p, rows, noise = PT.case_inputs(S, A, b, term)
        self.L = _lib.pretrain_layout(S, A)
        self.blob = packing.pack_pretrain(p, S, A, dev)
        self.blob_T = ops.pretrain_transpose(self.blob, S, A, precision=mode)
        self.is_param = packing.pack_pretrain({k: np.ones_like(v) for k, v in p.items()}, S, A, dev) != 0
        td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        s, a, s2, r = rows
        self.xenc, self.act, self.rew = td(np.concatenate([s, s2], 1)), td(a), td(r[..., 0])
        self.n6, self.n7 = td(np.stack(noise[:6])), td(noise[6])
        self.ws = ops.pretrain_workspace(S, A, b, dev)

    def za_region(self, use_trg):
        off = self.L.off_za_trg if use_trg else self.L.off_za_src
        return slice(off, off + 7 * self.L.za_member_floats)

    def grads(self, use_trg, b_global=None):
        ce, ct, cr = PT.TERMS[self.term]
        self.ws.fill_(float("nan"))
        grad = sentinel_blob(self.blob.numel(), self.dev)
        loss = torch.full((5,), float("nan"), device=self.dev)
        self.ops.pretrain_grads(self.S, self.A, self.b, use_trg, ce, self.blob, self.blob_T, self.xenc, self.act, self.rew, grad, loss,
                                self.ws, noise6=self.n6, noise7=self.n7, b_global=b_global, precision=self.mode,
                                transition_coef=ct, reward_coef=cr)
        torch.cuda.synchronize()
        return grad, loss.cpu().numpy().astype(np.float64)


def check_sentinels(c, grad, use_trg):
    bits = grad.view(torch.int32)
    other = c.za_region(not use_trg)
    assert bool((bits[other] == SENTINEL).all()), "the unused action encoder's gradient region was written"
    written = torch.ones_like(c.is_param)
    written[other] = False
    assert bool(torch.isfinite(grad[written]).all()), "a written gradient is not finite (or a float of the blob was not written)"
    pad = written & ~c.is_param
    assert not bool(grad[pad].any()), "layout padding of the gradient blob is not exactly 0"


def check_case(c, use_trg, b_global=None):
    S, A, b, term = c.S, c.A, c.b, c.term
    l64, g64, g32 = PT.reference(S, A, b, term, use_trg, b_global)
    grad, loss = c.grads(use_trg, b_global)
    check_sentinels(c, grad, use_trg)
    got = {k: v.cpu().numpy() for k, v in c.packing.unpack_pretrain(grad, S, A).items()}
    key = f"S{S}A{A}b{b}{'' if b_global is None else 'of%d' % b_global}/{term}/{'trg' if use_trg else 'src'}/{c.mode}"
    rec = RATIOS.setdefault(key, {})
    other = "za_src" if use_trg else "za_trg"
    for k, ref in g64.items():
        if k.startswith(other) or not PT.judged(term, k):
            continue
        half = k.startswith("za_") and k.split(".")[0].endswith("2")
        rec[k] = float("%.3g" % PT.rule_ratio(got[k + ".mu" if half else k], PT.blob_view(k, ref), PT.blob_view(k, g32[k])))
    print(key, "losses", loss, "worst", max(rec.items(), key=lambda kv: kv[1]))
    np.testing.assert_allclose(loss, l64, rtol=2e-5, atol=1e-7, err_msg=key)
    bad = {k: v for k, v in rec.items() if not v <= 1.0}
    assert not bad, (key, bad)


@pytest.mark.parametrize("term", list(PT.TERMS))
@pytest.mark.parametrize("geom", PT.GEOMETRIES, ids=lambda g: "S%dA%db%d" % g)
def test_term_gradients_vs_fp64(geom, term, dev, mfma):
    c = Case(*geom, term, mfma, dev)
    for use_trg in (False, True):
        check_case(c, use_trg)


@pytest.mark.parametrize("term", list(PT.TERMS))
def test_data_parallel_share_vs_fp64(term, dev, mfma):
    """b = 12 rows of a 24-row global batch: gradients and losses are the local share b / b_global of the global means."""
    c = Case(17, 6, 12, term, mfma, dev)
    for use_trg in (False, True):
        check_case(c, use_trg, b_global=24)


@pytest.mark.parametrize("use_trg", [False, True], ids=["src", "trg"])
@pytest.mark.parametrize("b", [12, 23, 32])
def test_fused_update_equals_grads_plus_adam(b, use_trg, dev, mfma):
    c = Case(17, 6, b, "all", mfma, dev)
    ops, lr = c.ops, 1e-3
    g = torch.Generator().manual_seed(b)
    m0 = (1e-3 * torch.randn(c.blob.numel(), generator=g)).to(dev)
    v0 = (1e-6 * torch.randn(c.blob.numel(), generator=g) ** 2).to(dev)
    out = []
    for fused in (True, False):
        blob, blob_T, m, v = c.blob.clone(), c.blob_T.clone(), m0.clone(), v0.clone()
        loss = torch.full((5,), float("nan"), device=dev)
        c.ws.fill_(float("nan"))
        if fused:
            ops.pretrain_update(c.S, c.A, b, use_trg, 1.0, blob, blob_T, c.xenc, c.act, c.rew, m, v, 3, 2, lr, loss, c.ws,
                                noise6=c.n6, noise7=c.n7, precision=mfma)
        else:
            grad = sentinel_blob(blob.numel(), dev)
            ops.pretrain_grads(c.S, c.A, b, use_trg, 1.0, blob, blob_T, c.xenc, c.act, c.rew, grad, loss, c.ws, noise6=c.n6,
                               noise7=c.n7, precision=mfma)
            ops.pretrain_adam(c.S, c.A, use_trg, blob, blob_T, grad, m, v, 3, 2, lr, precision=mfma)
        torch.cuda.synchronize()
        out.append(dict(blob=blob, m=m, v=v, blob_T=blob_T, loss_out=loss))
    moved = c.is_param.clone()
    moved[c.za_region(not use_trg)] = False
    assert bool(torch.isfinite(out[0]["blob"]).all()) and bool((out[0]["blob"] != c.blob)[moved].float().mean() > 0.99)
    assert torch.equal(out[0]["blob"][c.za_region(not use_trg)], c.blob[c.za_region(not use_trg)])      # Adam skips it
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), (k, int((out[0][k] != out[1][k]).sum()))
