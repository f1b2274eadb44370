"""The closed form of the level-0 Galerkin product at interior coarse points, restated in numpy and
compared with oracle/mg_prototype.py, float64 against float64.  No GPU: this pins the derivation, not the device code.

Every entry of a raw block (OF.py:843-960) is linear in nine per-pixel fields and the three constants alpha, beta, 1:
    S[m, oi, oj, t] = coefficient of field m in entry t = 3 r + c of the raw block of offset (oi, oj),
so at a coarse point C away from the border (prolongation weights 1 and 1/2 only, no ghost folds)
    4 A_c(C, C + (a, b))[t] = sum_f sum_m K[m, fi, fj, a, b, t] phi_m(2 C + (fi, fj)),
    K[m, fi, fj, a, b, t]   = w(fi) w(fj) sum_(oi, oj) S[m, oi, oj, t] w(fi + oi - 2 a) w(fj + oj - 2 b),
with w(0) = 1, w(+-1) = 1/2 and w = 0 elsewhere."""
import numpy as np
import pytest

from oracle import mg_prototype as mg, vof_oracle as orc

# fields: P P, P Dx, P Dy, P Dxx, P Dyy, P Dxy, P, Dx, Dy, then the constants alpha, beta, 1
PP, PDX, PDY, PDXX, PDYY, PDXY, P_, DX, DY, ALPHA, BETA, ONE = range(12)


def raw_block_coefficients():
    S = np.zeros((12, 3, 3, 9))
    c = S[:, 1, 1]                                        # offset (0, 0)
    c[PDXX, 0] = 1; c[PP, 0] = -2; c[ALPHA, 0] = -4
    c[PDXY, 1] = 1; c[PDXY, 3] = 1
    c[PDYY, 4] = 1; c[PP, 4] = -2; c[ALPHA, 4] = -4
    c[DX, 6] = 1; c[DY, 7] = 1
    c[ONE, 8] = -1; c[BETA, 8] = -4
    for s in (-1, 1):
        v = S[:, s + 1, 1]                                # offset (s, 0)
        v[PDX, 0] = s; v[PP, 0] = 1; v[ALPHA, 0] = 1
        v[PDY, 1] = s / 2; v[PDY, 3] = s / 2
        v[P_, 2] = -s / 2; v[P_, 6] = s / 2
        v[ALPHA, 4] = 1; v[BETA, 8] = 1
        h = S[:, 1, s + 1]                                # offset (0, s)
        h[ALPHA, 0] = 1
        h[PDX, 1] = s / 2; h[PDX, 3] = s / 2
        h[PDY, 4] = s; h[PP, 4] = 1; h[ALPHA, 4] = 1
        h[P_, 5] = -s / 2; h[P_, 7] = s / 2
        h[BETA, 8] = 1
        for s2 in (-1, 1):                                # the diagonals
            S[PP, s + 1, s2 + 1, 1] = s * s2 / 4
            S[PP, s + 1, s2 + 1, 3] = s * s2 / 4
    return S


def w(d):
    return {0: 1.0, -1: 0.5, 1: 0.5}.get(d, 0.0)


def closed_form_table(S):
    K = np.zeros((12, 3, 3, 3, 3, 9))
    for fi in (-1, 0, 1):
        for fj in (-1, 0, 1):
            for a in (-1, 0, 1):
                for b in (-1, 0, 1):
                    for oi in (-1, 0, 1):
                        for oj in (-1, 0, 1):
                            K[:, fi + 1, fj + 1, a + 1, b + 1] += (w(fi) * w(fj) * w(fi + oi - 2 * a) * w(fj + oj - 2 * b)) * S[:, oi + 1, oj + 1]
    return K


def fields(I, alpha, beta, quirks):
    d = orc.derivatives(I, I, quirks)
    P = d["P"]
    one = np.ones_like(P)
    return np.stack([P * P, P * d["Dx"], P * d["Dy"], P * d["Dxx"], P * d["Dyy"], P * d["Dxy"], P, d["Dx"], d["Dy"],
                     alpha * one, beta * one, one])


def interior_mask(nfi, nfj):
    """The kernel's interior test, as a mask over the coarse grid."""
    nci, ncj = mg.coarse_size(nfi), mg.coarse_size(nfj)
    cp, cq = np.meshgrid(np.arange(nci), np.arange(ncj), indexing="ij")
    return (cp >= 1) & (cp + 1 < nci) & (2 * cp + 1 <= nfi - 2) & (cq >= 1) & (cq + 1 < ncj) & (2 * cq + 1 <= nfj - 2)


def test_raw_block_coefficients_restate_the_fine_stencil():
    """S applied to the fields is the unfolded fine stencil of the oracle (so S is OF.py:843-960), and its non-zero pattern is
    the 43 entries the kernel's raw_block_mask names."""
    S = raw_block_coefficients()
    I = np.random.default_rng(5).random((9, 10)) * 2.0
    alpha, beta = 0.7, 3.0
    phi = fields(I, alpha, beta, True)
    raw = np.zeros((3, 3, 3, 3) + phi.shape[1:])
    for (rq, di, dj, cq, coef) in orc._interior_stencil(orc.derivatives(I, I, True), alpha, beta):
        raw[di + 1, dj + 1, rq, cq] += coef
    mine = np.einsum("mijt,mpq->ijtpq", S, phi).reshape(raw.shape)
    assert np.abs(mine - raw).max() <= 1e-14 * np.abs(raw).max()
    mask = {(0, 0): 0x1DB, (1, 0): 0x15F, (0, 1): 0x1BB, (1, 1): 0x00A}
    for oi in (-1, 0, 1):
        for oj in (-1, 0, 1):
            bits = sum(1 << t for t in range(9) if np.any(S[:, oi + 1, oj + 1, t] != 0))
            assert bits == mask[(abs(oi), abs(oj))]
    assert sum(bin(mask[(abs(oi), abs(oj))]).count("1") for oi in (-1, 0, 1) for oj in (-1, 0, 1)) == 43


@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("alpha,beta", [(1.0, 1e4), (0.3, 2.0)])
@pytest.mark.parametrize("shape", [(12, 13), (21, 20)])
def test_closed_form_is_the_interior_level1_stencil(shape, alpha, beta, quirks):
    I = np.random.default_rng(shape[0] * 100 + shape[1]).random(shape) * 2.0
    K = closed_form_table(raw_block_coefficients())
    phi = fields(I, alpha, beta, quirks)
    nfi, nfj = phi.shape[1:]
    ref = mg.Hierarchy(I, alpha, beta, quirks).levels[1]            # [a, b, r, c, cp, cq]
    nci, ncj = ref.shape[-2:]
    inside = interior_mask(nfi, nfj)
    assert inside.any()
    mine = np.zeros((3, 3, 9, nci, ncj))
    for cp, cq in zip(*np.nonzero(inside)):
        patch = phi[:, 2 * cp - 1:2 * cp + 2, 2 * cq - 1:2 * cq + 2]           # [m, fi, fj]
        mine[:, :, :, cp, cq] = 0.25 * np.einsum("mijabt,mij->abt", K, patch)
    mine = mine.reshape(ref.shape)
    a, b = mine[..., inside], ref[..., inside]
    assert np.linalg.norm(a - b) / np.linalg.norm(b) <= 1e-12


def test_constant_part_and_vanishing_terms():
    """What the kernel relies on: the alpha / beta / 1 part of an interior point does not depend on the image (the sum of K over
    the nine fine points), and many K vanish (antisymmetry of the first-derivative terms, raw_block_mask)."""
    K = closed_form_table(raw_block_coefficients())
    Kc = K[ALPHA:].sum(axis=(1, 2))                                            # [alpha / beta / 1, a, b, t]
    # an image-free operator: the constant-coefficient 5-point Laplacians, averaged
    assert np.isclose(Kc[0, :, :, 0].sum(), 0.0) and np.isclose(Kc[0, :, :, 4].sum(), 0.0)   # alpha rows sum to zero
    assert np.isclose(Kc[1, :, :, 8].sum(), 0.0)                                                # beta row likewise
    assert np.isclose(Kc[2, :, :, 8].sum(), -4.0)                                               # 4 x the screening term -1
    # the counts the kernel's comment and DESIGN.md state: image terms of the 9 x 9 x 81; coefficients of the constant part and
    # the entries of the 81 they sit on
    assert np.count_nonzero(K[:ALPHA]) == 552
    assert np.count_nonzero(Kc) == 36 and np.count_nonzero((Kc != 0).any(axis=0)) == 27
