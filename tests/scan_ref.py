"""The integer oracle of ntt_batch_inverse and ntt_matrix_scan: Python integers over F_p[X]/(X^d - W), restating
include/ntt.h's definitions and nothing of the kernels' order of operations.  A matrix is a numpy array
[rows][width * d] of canonical values; the scans are plain loops over the rows, vectorised over the columns with
object arrays; the inverse is defined by a * a^-1 = 1 and 0 -> 0."""
import numpy as np

from tests.test_gpu_fold import _ext_mul


def ext_mul_vec(a, b, w, p):
    """a b element by element for a, b = [count][d] object arrays."""
    d = a.shape[1]
    out = np.zeros_like(a)
    for i in range(d):
        for j in range(d):
            t = a[:, i] * b[:, j]
            if i + j < d:
                out[:, i + j] += t
            else:
                out[:, i + j - d] += t * w
    return out % p


def identity(width, d, op):
    one = np.zeros((width, d), dtype=object)
    if op == "product":
        one[:, 0] = 1
    return one


def scan(mat, width, d, w, p, op):
    """(inclusive, exclusive, totals) of mat = [rows][width * d]: out[i][j] = (+)_{r <= i} (r < i) mat[r][j]."""
    rows = mat.shape[0]
    m = mat.astype(object).reshape(rows, width, d)
    inc = np.zeros((rows, width, d), dtype=object)
    exc = np.zeros((rows, width, d), dtype=object)
    acc = identity(width, d, op)
    for r in range(rows):
        exc[r] = acc
        acc = (acc + m[r]) % p if op == "sum" else ext_mul_vec(acc, m[r], w, p)
        inc[r] = acc
    return inc.reshape(rows, width * d), exc.reshape(rows, width * d), acc.reshape(width * d)


def scan_one_column(col, p, op):
    """The same for one base column of Python ints (the long case): plain integers, no arrays."""
    inc, exc, acc = [], [], 1 if op == "product" else 0
    for v in col:
        exc.append(acc)
        acc = (acc + v) % p if op == "sum" else acc * v % p
        inc.append(acc)
    return inc, exc, acc


def ext_inverse(a, w, p):
    """a^-1 for one element (a list of d ints); 0 -> 0.  d = 1: Fermat; else the solution of the d x d system."""
    d = len(a)
    if not any(a):
        return [0] * d
    if d == 1:
        return [pow(a[0], p - 2, p)]
    # columns of the multiplication-by-a matrix: a X^j
    cols = [_ext_mul(a, [1 if i == j else 0 for i in range(d)], w, p) for j in range(d)]
    M = [[cols[j][i] for j in range(d)] + [1 if i == 0 else 0] for i in range(d)]
    for c in range(d):  # Gauss-Jordan mod p
        piv = next(r for r in range(c, d) if M[r][c])
        M[c], M[piv] = M[piv], M[c]
        inv = pow(M[c][c], p - 2, p)
        M[c] = [v * inv % p for v in M[c]]
        for r in range(d):
            if r != c and M[r][c]:
                f = M[r][c]
                M[r] = [(x - f * y) % p for x, y in zip(M[r], M[c])]
    return [M[i][d] for i in range(d)]


def is_inverse(x, y, d, w, p):
    """y is the inverse of x = [count][d] element by element: x y = 1 where x != 0, y = 0 where x = 0."""
    xo, yo = x.astype(object).reshape(-1, d), y.astype(object).reshape(-1, d)
    zero = ~np.array([any(r) for r in xo], dtype=bool)
    prod = ext_mul_vec(xo, yo, w, p)
    one = np.zeros_like(prod)
    one[~zero, 0] = 1
    return bool((prod == one).all()) and not bool(np.array([any(r) for r in yo[zero]], dtype=bool).any())
