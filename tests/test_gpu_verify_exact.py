"""Batch verification's two random linear combinations, EXACTLY: verify_phase1_dev / verify_session_zy / verify_phase2_dev on
batches built by tests/verify_exact.py, whose points have known discrete logs and whose blobs are polynomials of degree <= 7,
so that z_i, y_i, the transcript roots and both partial sums (src/kzg/setup.rs:151-160) are known from Python integers.

The sizes walk every row of choose_var_geom (engine_verify.hip): A has n terms and B 2 n + 1, c = 4 below 64 terms, c = 8
below 32,768, the flat path (c = 13, balanced shares + fix-up pass, bit sums, host Horner) from there on -- 16,384 ... 32,767
items is the row where B is flat and A is not; 65,537 items is the first size whose exponents use bit 16 and whose transcript
has a 257th group.  At three sizes the same batches also go through contexts built with every knob that changes the lincombs'
or phase 1's kernels, and the 65,537 batch is cut into shares (phase 2 with all roots and each share's first_index: the group
path's and dist.py's phase 2)."""
import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

import verify_exact as vx  # noqa: E402

N_MAX = 65537
SIZES = (2, 31, 32, 63, 64, 16383, 16384, 32767, 32768, 40961, 65536, 65537)
CLEAN = [-1, 0, -1, 0, -1, 0]
# contexts made with one knob each, at 16,384, 32,768 and 65,537 items
VARIANTS = {
    "seg_per_bucket": {"KATETH_AMD_VAR_SEG": "0"},  # the flat path with one thread per bucket
    "seg16": {"KATETH_AMD_VAR_SEG": "16"},  # other share sizes for k_var_buckets_seg / k_var_seg_fixup
    "seg17": {"KATETH_AMD_VAR_SEG": "17"},
    "seg4096": {"KATETH_AMD_VAR_SEG": "4096"},
    "classic": {"KATETH_AMD_VAR_MSM": "classic"},  # c = 8 everywhere; at 65,537 items 64 partials per bucket
    "glv": {"KATETH_AMD_VAR_GLV": "1"},
    # the one-lane-per-blob hash at 32,768 and the 64-lane evaluation on full-chip batches
    "hash_one_lane_eval64": {"KATETH_AMD_CHALLENGE_SPLIT_MAX": "1", "KATETH_AMD_EVAL_GROUP": "64"},
    # the producer/consumer hash at 65,537
    "hash_pairs_eval16": {"KATETH_AMD_CHALLENGE_SPLIT_MAX": "1000000", "KATETH_AMD_EVAL_GROUP": "16"},
}
VARIANT_SIZES = (16384, 32768, 65537)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def engine():
    import kateth_amd

    s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    yield s
    s.close()


@pytest.fixture(scope="module")
def batches():
    return {"walk": vx.Batch(N_MAX, seed=0xE4AC7), "tiny": vx.Batch(N_MAX, seed=0x711E, tiny=True)}


@pytest.fixture(scope="module")
def dev(torch_cuda, batches):
    """the tiled blobs (item i = blob i % 7) and both point sets on the device, N_MAX items each"""
    import numpy as np

    torch = torch_cuda
    torch.cuda.empty_cache()
    b = batches["walk"]
    tiles = torch.from_numpy(np.frombuffer(b"".join(b.blobs), dtype=np.uint8).copy()).view(vx.NBLOBS, vx.BLOB_BYTES).cuda()
    d = {"blobs": tiles[torch.arange(N_MAX, device="cuda") % vx.NBLOBS].contiguous()}
    del tiles
    for key, bb in batches.items():
        assert bb.blobs == b.blobs
        d[key] = tuple(torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda() for x in (bb.com, bb.prf))
    torch.cuda.synchronize()
    yield d
    d.clear()
    torch.cuda.empty_cache()


def _same_items(got, want, width, what, base):
    if got == want:
        return
    bad = [k for k in range(len(want) // width) if got[width * k:width * k + width] != want[width * k:width * k + width]]
    pytest.fail("%s: %d items differ, the first at global index %d" % (what, len(bad), base + bad[0]) if bad else "%s: length" % what)


def _check(e, dev, b, key, shares, label):
    """phase 1 per share, z / y of every item, the roots, then phase 2 per share with all roots: each share's 192 bytes must be
    the builder's exact sums over that share's global range"""
    blobs = dev["blobs"].data_ptr()
    d_c, d_p = (t.data_ptr() for t in dev[key])
    want_roots, _, want_parts = b.expect(shares)
    n_total = shares[-1][1]
    sessions, roots = [], []
    try:
        for lo, hi in shares:
            sess, root, err = e.verify_phase1_dev(blobs + lo * vx.BLOB_BYTES, d_c + 48 * lo, d_p + 48 * lo, hi - lo)
            sessions.append(sess)
            assert err == CLEAN, (label, lo, err)
            zs, ys = e.verify_session_zy(sess, 0, hi - lo)
            _same_items(zs, b.zb[32 * lo:32 * hi], 32, "%s: z" % label, lo)
            _same_items(ys, b.yb[32 * lo:32 * hi], 32, "%s: y" % label, lo)
            roots.append(root)
        assert roots == want_roots, label
        got = [e.verify_phase2_dev(sess, b"".join(roots), lo, n_total) for sess, (lo, _) in zip(sessions, shares)]
    finally:
        for sess in sessions:
            e.verify_session_destroy(sess)
    for (lo, hi), g, w in zip(shares, got, want_parts):
        assert g[:96] == w[:96], "%s: A of items [%d, %d) of %d" % (label, lo, hi, n_total)
        assert g[96:] == w[96:], "%s: B of items [%d, %d) of %d" % (label, lo, hi, n_total)


@pytest.mark.parametrize("n", SIZES)
def test_exact_lincombs_default_context(n, engine, dev, batches):
    _check(engine, dev, batches["walk"], "walk", [(0, n)], "default n=%d" % n)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_exact_lincombs_with_knobs(variant, dev, batches, monkeypatch):
    """environment knobs are read once, at kzg_ctx_create: a context per setting"""
    import kateth_amd

    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    e = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        for n in VARIANT_SIZES:
            _check(e, dev, batches["walk"], "walk", [(0, n)], "%s n=%d" % (variant, n))
    finally:
        e.close()


@pytest.mark.parametrize("n", [33000, 65537])
def test_exact_lincombs_on_a_tiny_point_set(n, engine, dev, batches):
    """every point one of +-[1..8]G: bucket chains add P + P and P + (-P) and restart from the identity partway through"""
    _check(engine, dev, batches["tiny"], "tiny", [(0, n)], "tiny n=%d" % n)


@pytest.mark.parametrize("cuts", [(16384,), (21001, 43223)], ids=["2shares", "3shares"])
def test_exact_partial_sums_of_shares(cuts, engine, dev, batches):
    """the 65,537 batch in shares: one phase-1 session per share, phase 2 with all roots and each share's first_index"""
    edges = (0,) + cuts + (N_MAX,)
    _check(engine, dev, batches["walk"], "walk", list(zip(edges, edges[1:])), "shares %s" % (cuts,))
