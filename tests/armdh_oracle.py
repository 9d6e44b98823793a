"""TEST ORACLE of BatchArmDH: a plain-Python restatement of transformation_matrix, forward_kinematics, basic_jacobian, the pose
functions and inverse_kinematics of 01_forward_inverse_kinematics.py, with the arithmetic forms numpy takes written out on Python
floats: np.dot of two 4 x 4 matrices as acc = fma(A[i][k], B[k][j], acc) from 0.0, np.cross as multiply, multiply, subtract.

The step is NOT the reference's: step_newton and step_lm are this package's own definition, operation for operation what the top
of csrc/rpp_armdh.h states (tests/test_armdh_host.py holds the two bit-identical, and measures the step against the reference's
recorded one)."""
import ctypes
import ctypes.util
import math
import struct
from fractions import Fraction

OK, NONFINITE, NO_CONVERGENCE = 0, 1, 2
MAX_SWEEPS = 30
PAIR_EPS = 2.0 ** -50
ROW_EPS = 2.0 ** -120
CUT = 1e-15
PI = math.pi
HALF_PI = math.pi / 2
TRIG_MAX = struct.unpack("<d", struct.pack("<Q", 0x419921FB << 32))[0]   # where the device's libm replicas end


def _fma_function():
    if hasattr(math, "fma"):
        return math.fma
    try:
        f = ctypes.CDLL(ctypes.util.find_library("m")).fma
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_double] * 3
        if f(0.1, 10.0, -1.0) == float(Fraction(0.1) * 10 - 1):
            return f
    except (OSError, AttributeError, TypeError):
        pass
    return lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c))


fma = _fma_function()


def sq(x):
    """x ** 2 as the interpreter computes it"""
    return float(x) ** 2


def sqrt(x):
    """IEEE: NaN where math.sqrt raises"""
    return math.sqrt(x) if x >= 0.0 else math.nan


def dot4(A, B):
    C = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = fma(A[i][k], B[k][j], acc)
            C[i][j] = acc
    return C


def dot4_unfused(A, B):
    """The form np.dot is NOT: products and sums rounded one by one, left to right"""
    return [[((A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]) + A[i][3] * B[3][j] for j in range(4)] for i in range(4)]


def local_matrix(row):
    th, al, a, d = row
    st, ct, sa, ca = math.sin(th), math.cos(th), math.sin(al), math.cos(al)
    return [[ct, (-st) * ca, st * sa, a * ct], [st, ct * ca, (-ct) * sa, a * st], [0.0, sa, ca, d], [0.0, 0.0, 0.0, 1.0]]


def cross(z, d):
    return [z[1] * d[2] - z[2] * d[1], z[2] * d[0] - z[0] * d[2], z[0] * d[1] - z[1] * d[0]]


def forward(dh):
    """-> (globals [N] of 4 x 4, J [6][N]) or None when a theta is not finite or lies at or beyond TRIG_MAX"""
    n = len(dh)
    T = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    glob, prev = [], []
    for row in dh:
        if not abs(row[0]) < TRIG_MAX:
            return None
        prev.append(([T[0][3], T[1][3], T[2][3]], [T[0][2], T[1][2], T[2][2]]))
        T = dot4(T, local_matrix(row))
        glob.append(T)
    ee = [T[0][3], T[1][3], T[2][3]]
    J = [[0.0] * n for _ in range(6)]
    for l, (o, z) in enumerate(prev):
        c = cross(z, [ee[0] - o[0], ee[1] - o[1], ee[2] - o[2]])
        for r in range(3):
            J[r][l] = c[r]
            J[3 + r][l] = z[r]
    return glob, J


def rot2euler2(T):
    alpha = math.atan2(T[1][2], T[0][2])
    if not (-HALF_PI <= alpha <= HALF_PI):
        alpha = math.atan2(T[1][2], T[0][2]) + PI
    if not (-HALF_PI <= alpha <= HALF_PI):
        alpha = math.atan2(T[1][2], T[0][2]) - PI
    sA, cA = math.sin(alpha), math.cos(alpha)
    beta = math.atan2(T[0][2] * cA + T[1][2] * sA, T[2][2])
    gamma = math.atan2((-T[0][0]) * sA + T[1][0] * cA, (-T[0][1]) * sA + T[1][1] * cA)
    return alpha, beta, gamma


def rot2euler(T):
    flag = -1.0 if T[0][3] < 0 else 1.0
    return (math.atan2(flag * sqrt(sq(T[0][2]) + sq(T[1][2])), T[2][2]), math.atan2(flag * T[1][2], flag * T[0][2]),
            math.atan2(flag * T[2][1], (-1.0 * flag) * T[2][0]))


def rot2quat(T):
    flag = -1.0 if T[0][3] < 0 else 1.0
    qw = 0.5 * sqrt(((1.0 + T[0][0]) + T[1][1]) + T[2][2])
    den = 4.0 * qw

    def div(a):
        if den == 0.0:
            return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, den)
        return a / den
    return qw, div(flag * (T[2][1] - T[1][2])), div(flag * (T[0][2] - T[2][0])), div(flag * (T[1][0] - T[0][1]))


def quat2rpy(q):
    qw, qx, qy, qz = q
    if not all(math.isfinite(v) for v in q):
        return math.nan, math.nan, math.nan   # only checked where the reference's own values are finite
    return (math.atan2(2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (sq(qx) + sq(qy))),
            math.atan2(-2.0 * (qx * qz - qw * qy), sqrt(4.0 * sq(qy * qz + qw * qx) + sq(1.0 - 2.0 * (sq(qx) + sq(qy))))),
            math.atan2(2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (sq(qy) + sq(qz))))


def pose_of(T):
    a, b, g = rot2euler2(T)
    return [T[0][3], T[1][3], T[2][3], a, b, g]


def kzyz(alpha, beta):
    sA, cA, sB, cB = math.sin(alpha), math.cos(alpha), math.sin(beta), math.cos(beta)
    return [[0.0, -sA, cA * sB], [0.0, cA, sA * sB], [1.0, 0.0, cB]]


def e_of(K, diff):
    return list(diff[:3]) + [(K[r][0] * diff[3] + K[r][1] * diff[4]) + K[r][2] * diff[5] for r in range(3)]


def step_newton(J, e):
    """-> (delta or None, status, kappa, cut, sigma [6], kept [6]): J is not changed"""
    n = len(J[0])
    A = [list(r) for r in J]
    V = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    F = 0.0
    for r in range(6):
        for k in range(n):
            F = F + A[r][k] * A[r][k]
    floor = ROW_EPS * F
    rotated = True
    sweep = 0
    while sweep < MAX_SWEEPS and rotated:
        rotated = False
        for p in range(5):
            for q in range(p + 1, 6):
                a = b = c = 0.0
                for k in range(n):
                    u, v = A[p][k], A[q][k]
                    a = a + u * u
                    b = b + v * v
                    c = c + u * v
                if c == 0.0 or abs(c) <= PAIR_EPS * math.sqrt(a * b) or a <= floor or b <= floor:
                    continue
                rotated = True
                zeta = (b - a) / (2.0 * c)
                t = (-1.0 if zeta < 0.0 else 1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / math.sqrt(1.0 + t * t)
                sn = cs * t
                for k in range(n):
                    u, v = A[p][k], A[q][k]
                    A[p][k] = cs * u - sn * v
                    A[q][k] = sn * u + cs * v
                for r in range(6):
                    u, v = V[r][p], V[r][q]
                    V[r][p] = cs * u - sn * v
                    V[r][q] = sn * u + cs * v
        sweep += 1
    if rotated:
        return None, NO_CONVERGENCE, 0.0, False, None, None
    s2 = []
    for i in range(6):
        a = 0.0
        for k in range(n):
            a = a + A[i][k] * A[i][k]
        s2.append(a)
    sg = [math.sqrt(a) for a in s2]
    smax = max(sg)
    keep = [sg[i] > CUT * smax for i in range(6)]
    w = [0.0] * 6
    for i in range(6):
        dot = 0.0
        for r in range(6):
            dot = dot + V[r][i] * e[r]
        if keep[i]:
            w[i] = dot / s2[i]
    delta = []
    for k in range(n):
        acc = 0.0
        for i in range(6):
            if keep[i]:
                acc = acc + A[i][k] * w[i]
        delta.append(acc)
    kept = [sg[i] for i in range(6) if keep[i]]
    kappa = smax / min(kept) if kept else 0.0
    return delta, OK, kappa, len(kept) < min(6, n), sg, keep


def lm_system(J, K, diff, eps):
    """-> (M lower triangle as rows, rhs)"""
    n = len(J[0])
    W = [1.0, 1.0, 1.0, HALF_PI, HALF_PI, HALF_PI]
    jv = [list(J[r]) for r in range(3)] + [[(K[r][0] * J[3][k] + K[r][1] * J[4][k]) + K[r][2] * J[5][k] for k in range(n)] for r in range(3)]
    M, rhs = [], []
    for i in range(n):
        wi = [jv[r][i] * W[r] for r in range(6)]
        row = []
        for j in range(i + 1):
            acc = 0.0
            for r in range(6):
                acc = acc + wi[r] * jv[r][j]
            row.append(acc + eps if i == j else acc)
        M.append(row)
        acc = 0.0
        for r in range(6):
            acc = acc + wi[r] * diff[r]
        rhs.append(acc)
    return M, rhs


def step_lm(J, K, diff, eps):
    """-> (delta or None, status)"""
    n = len(J[0])
    L, x = lm_system(J, K, diff, eps)
    for j in range(n):
        d = L[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 0.0:
            return None, NO_CONVERGENCE
        d = math.sqrt(d)
        L[j][j] = d
        for i in range(j + 1, n):
            v = L[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / d
    for i in range(n):
        v = x[i]
        for k in range(i):
            v = v - L[i][k] * x[k]
        x[i] = v / L[i][i]
    for i in range(n - 1, -1, -1):
        v = x[i]
        for k in range(i + 1, n):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    return x, OK


def step(J, K, diff, method="newton", eps=1e-5):
    """-> (delta or None, status, kappa, cut)"""
    if method == "lm":
        d, st = step_lm(J, K, diff, eps)
        return d, st, 0.0, False
    d, st, kappa, cut, _, _ = step_newton(J, e_of(K, diff))
    return d, st, kappa, cut


def forward_record(dh):
    """What BatchArmDH.forward reports of one arm: dict(status, transforms, J, pos, euler2, euler, quat, rpy)"""
    f = forward(dh)
    if f is None:
        return dict(status=NONFINITE)
    glob, J = f
    T = glob[-1]
    q = rot2quat(T)
    return dict(status=OK, transforms=glob, J=J, pos=[T[0][3], T[1][3], T[2][3]], euler2=list(rot2euler2(T)), euler=list(rot2euler(T)),
                quat=list(q), rpy=list(quat2rpy(q)))


def solve(dh, ref, iter_cnt=500, step_div=200.0, method="newton", eps=1e-5):
    """-> dict(status, angles, pose, pose_error, kappa_max, n_cut): inverse_kinematics :387-438 without the drawing, then one more
    forward pass"""
    dh = [[float(v) for v in row] for row in dh]
    ref = [float(v) for v in ref]
    n = len(dh)
    status, kappa_max, n_cut = OK, 0.0, 0
    for _ in range(iter_cnt):
        f = forward(dh)
        if f is None:
            status = NONFINITE
            break
        glob, J = f
        pose = pose_of(glob[-1])
        diff = [ref[r] - pose[r] for r in range(6)]
        delta, status, kappa, cut = step(J, kzyz(pose[3], pose[4]), diff, method, eps)
        if status != OK:
            break
        kappa_max = max(kappa_max, kappa)
        n_cut += 1 if cut else 0
        for k in range(n):
            dh[k][0] = dh[k][0] + delta[k] / step_div
        if not all(math.isfinite(row[0]) for row in dh):
            status = NONFINITE
            break
    f = forward(dh)
    if f is None:
        status, pose = NONFINITE, [0.0] * 6
    else:
        pose = pose_of(f[0][-1])
    return dict(status=status, angles=[row[0] for row in dh], pose=pose, pose_error=[ref[r] - pose[r] for r in range(6)],
                kappa_max=kappa_max, n_cut=n_cut)
