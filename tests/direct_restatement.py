"""Plain float64 restatement (numpy / scipy) of the direct preconditioner of csrc/vof_direct.hpp - the block-tridiagonal LU of the
level-0 operator by image rows - and of the rule that picks the kernel which inverts its Schur blocks (direct_uses_blocked /
direct_ld of csrc/vof.hip).  tests/test_direct_restatement_cpu.py checks it against a sparse direct solve;
tests/test_gpu_direct_pin.py holds the library's one-step residual against it.

With the unknowns of image row p as one block, in the order (field, q), the folded 9-point operator is block tridiagonal,
A = tridiag(L_p, D_p, U_p).  Block elimination
    S_0 = D_0,   S_p = D_p - L_p T_{p-1} U_{p-1},   T_p = S_p^-1,
then z = A^-1 r by  y_p = r_p - L_p T_{p-1} y_{p-1}  (forward)  and  x_p = T_p (y_p - U_p x_{p+1})  (backward).

Two inverses: numpy's (LAPACK: what the method can reach) and `tile_inverse`, which restates the design of the blocked kernels
(what the design can reach without pivoting across tiles).  The quantity the tests compare is the TRUE residual
||b - A x|| / ||b|| after one Krylov step: with an exact M^-1 the first BiCGStab half-step lands on the solution, so that residual
measures how exact M^-1 is.  (The recursively updated residual of the iteration does not: it is zero by construction when the step ends,
whatever M^-1 was; at the ill-conditioned case of tests/direct_cases.py it reads 1e-19 where the true one is 3e-11.)

No elimination can leave less than rounding allows: a backward stable solve of A x = b ends with a residual of the order of
eps ||A|| ||x|| / ||b|| (`attainable`), times a growth factor.  In the grad-div dominated corner (8-bit data, alpha 0.3, beta 0.1)
that level is 3e-12 ... 1e-10, and a one-step residual lands anywhere between 1e-13 and 5e-11 with either inverse, depending on the
stack and on the summation order: there the level, not the other inverse, is the yardstick."""
import numpy as np
import scipy.sparse.linalg

from oracle import mg_prototype as mg
from oracle import vof_oracle as orc

TILE = 64           # DNB: tile size of the blocked Gauss-Jordan inverse (csrc/vof_direct.hpp)
OWN_MAX = 192       # DIRECT_OWN_MAX: largest m the one-workgroup inverse k_dir_invert takes (csrc/vof.hip)


def path_rule(N_j):
    """The inverse an image of N_j columns takes: m = 3 n_j unknowns per image row (n_j = N_j - 2 interior columns); blocked iff
    m > OWN_MAX; ld = m rounded up to a multiple of TILE when blocked (identity padding), else m; nt = ld / TILE tiles per side
    (0 on the one-workgroup path, which has no tiles)."""
    m = 3 * (N_j - 2)
    blocked = m > OWN_MAX
    ld = -(-m // TILE) * TILE if blocked else m
    return dict(m=m, blocked=blocked, ld=ld, nt=ld // TILE if blocked else 0)


def tile_inverse(S):
    """Inverse of S as the blocked kernels form it: padded with the identity to a multiple of TILE, block Gauss-Jordan over
    TILE x TILE tiles, every diagonal tile inverted on its own (pivoting inside the tile only, none across tiles):
        D = A[k,k]^-1,  R = D A[k,:],  C = A[:,k],  A -= C R,  A[:,k] = -C D,  A[k,:] = R,  A[k,k] = D   for every tile index k."""
    m = S.shape[0]
    ld = -(-m // TILE) * TILE
    A = np.eye(ld)
    A[:m, :m] = S
    for k in range(ld // TILE):
        ks = slice(k * TILE, (k + 1) * TILE)
        D = np.linalg.inv(A[ks, ks])
        R = D @ A[ks, :]
        C = A[:, ks].copy()
        A -= C @ R
        A[:, ks] = -C @ D
        A[ks, :] = R
        A[ks, ks] = D
    return A[:m, :m]


INVERSES = {"lapack": np.linalg.inv, "tile": tile_inverse}


class RowBlockLU:
    """M^-1 of the interior system A (csr, unknowns ordered (field, p, q)) of an n_i x n_j interior grid."""

    def __init__(self, A, n_i, n_j, inverse):
        inv = INVERSES[inverse] if isinstance(inverse, str) else inverse
        A = A.tocsr()
        N = n_i * n_j
        # unknowns of image row p in the order (field, q)
        self.idx = np.array([[f * N + p * n_j + q for f in range(3) for q in range(n_j)] for p in range(n_i)])
        rows = [A[ix] for ix in self.idx]
        blk = lambda p, p2: rows[p][:, self.idx[p2]].toarray()
        self.L = [None] + [blk(p, p - 1) for p in range(1, n_i)]
        self.U = [blk(p, p + 1) for p in range(n_i - 1)] + [None]
        self.T = []
        for p in range(n_i):
            S = blk(p, p)
            if p > 0:
                S = S - self.L[p] @ (self.T[p - 1] @ self.U[p - 1])
            self.T.append(inv(S))
        self.n_i = n_i

    def solve(self, r):
        n_i, idx, L, U, T = self.n_i, self.idx, self.L, self.U, self.T
        shape = r.shape
        r = r.ravel()
        y = [None] * n_i
        x = [None] * n_i
        for p in range(n_i):
            y[p] = r[idx[p]] - (L[p] @ (T[p - 1] @ y[p - 1]) if p > 0 else 0.0)
        for p in range(n_i - 1, -1, -1):
            x[p] = T[p] @ (y[p] - (U[p] @ x[p + 1] if p + 1 < n_i else 0.0))
        z = np.empty_like(r)
        for p in range(n_i):
            z[idx[p]] = x[p]
        return z.reshape(shape)


def system(I, J, alpha, beta, quirks=True):
    """(A, b) of the interior system of the pair (I, J): A sparse with unknowns (field, p, q), b flat in the same order."""
    A = mg.stencil_to_sparse(mg.fine_stencil(I, alpha, beta, quirks))
    b = orc.rhs_interior(np.asarray(I, dtype=np.float64), np.asarray(J, dtype=np.float64), quirks).ravel()
    return A, b


def attainable(A, b):
    """eps ||A|| ||x|| / ||b|| with x the sparse direct solution and ||A|| = sqrt(||A||_1 ||A||_inf) >= ||A||_2: the residual level
    rounding alone leaves in a backward stable solve."""
    x = scipy.sparse.linalg.splu(A.tocsc()).solve(b)
    norm_A = np.sqrt(scipy.sparse.linalg.norm(A, 1) * scipy.sparse.linalg.norm(A, np.inf))
    return float(np.finfo(np.float64).eps * norm_A * np.linalg.norm(x) / np.linalg.norm(b))


def one_step(I, J, alpha, beta, quirks=True, x0=None, inverse="lapack", rtol=1e-10):
    """One BiCGStab step (oracle/mg_prototype.py, max_it = 1) preconditioned by the restated M^-1.  Returns x as (3, n_i, n_j), the
    step count and the TRUE relative residual ||b - A x|| / ||b|| (not the iteration's recursively updated one)."""
    A, b = system(I, J, alpha, beta, quirks)
    n_i, n_j = I.shape[0] - 2, I.shape[1] - 2
    lu = RowBlockLU(A, n_i, n_j, inverse)
    x, it, _hist = mg.bicgstab(lambda v: A @ v, lu.solve, b, x0=None if x0 is None else np.asarray(x0, dtype=np.float64).ravel(),
                               rtol=rtol, max_it=1)
    true_rr = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    return x.reshape(3, n_i, n_j), it, true_rr
