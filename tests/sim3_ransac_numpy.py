"""An independent numpy restatement of Sim3Solver (reference src/Sim3Solver.cc) as csrc/sim3_ransac.h defines its arithmetic:
ComputeSim3 with np.linalg.eigh in float64 on the float32 N (LAPACK, not the header's Jacobi method), the float32 statements as
explicit np.float32 operations, CheckInliers, the record scan, and `replay`: the reference's iterate loop one iteration at a time."""
import numpy as np

F = np.float32
PINHOLE, KB8 = 0, 1


def centroid(P):
    """P [3 points, 3] float32 -> relative coordinates, centroid (:302-308)."""
    P = np.asarray(P, F)
    C = ((P[0] + P[1]) + P[2]) / F(3)
    return (P - C).astype(F), C.astype(F)


def horn_matrix(Pr1, Pr2):
    """The float32 N (:328-349): M in float32, the ten entries in float64, rounded once."""
    M = np.zeros((3, 3), F)
    for i in range(3):
        for j in range(3):
            M[i, j] = (Pr2[0, i] * Pr1[0, j] + Pr2[1, i] * Pr1[1, j]) + Pr2[2, i] * Pr1[2, j]
    m = M.astype(np.float64)
    N11, N12, N13, N14 = m[0, 0] + m[1, 1] + m[2, 2], m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]
    N22, N23, N24 = m[0, 0] - m[1, 1] - m[2, 2], m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]
    N33, N34, N44 = -m[0, 0] + m[1, 1] - m[2, 2], m[1, 2] + m[2, 1], -m[0, 0] - m[1, 1] + m[2, 2]
    return np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]).astype(F)


def top_quaternion(N):
    """The unit eigenvector (w, x, y, z) of the largest eigenvalue of the float32 N, w >= 0: LAPACK in float64."""
    w, v = np.linalg.eigh(np.asarray(N, F).astype(np.float64))
    q = v[:, np.argmax(w)]
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def quaternion_rotation(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]).astype(F)


def compute_sim3(P1, P2, fix_scale):
    """The 13 floats R, t, s of the minimal set P1, P2 [3 points, 3]."""
    Pr1, O1 = centroid(P1)
    Pr2, O2 = centroid(P2)
    R = quaternion_rotation(top_quaternion(horn_matrix(Pr1, Pr2)))
    s = F(1)
    if not fix_scale:
        nom, den = F(0), F(0)
        for k in range(3):
            for i in range(3):
                p3 = (R[i, 0] * Pr2[k, 0] + R[i, 1] * Pr2[k, 1]) + R[i, 2] * Pr2[k, 2]
                nom = nom + Pr1[k, i] * p3
                den = den + p3 * p3
        with np.errstate(all="ignore"):
            s = F(np.float64(nom) / np.float64(den))
    with np.errstate(all="ignore"):
        sR = (s * R).astype(F)
        t = np.array([O1[i] - ((sR[i, 0] * O2[0] + sR[i, 1] * O2[1]) + sR[i, 2] * O2[2]) for i in range(3)], F)
    return np.concatenate([R.reshape(9), t, [s]]).astype(F)


def transforms(T13):
    """sR, t, sRinv, tinv of R, t, s (:398-411)."""
    T13 = np.asarray(T13, F)
    R, t, s = T13[:9].reshape(3, 3), T13[9:12], T13[12]
    with np.errstate(all="ignore"):
        sinv = F(np.float64(1.0) / np.float64(s))
        sR = (s * R).astype(F)
        sRinv = (sinv * R.T).astype(F)
        tinv = np.array([-((sRinv[i, 0] * t[0] + sRinv[i, 1] * t[1]) + sRinv[i, 2] * t[2]) for i in range(3)], F)
    return sR, t, sRinv, tinv


def project(camera_type, cam, sR, t, X):
    """Project (:461-475) of the points X [n, 3] float32: [n, 2] float32."""
    cam = np.asarray(cam, F)
    with np.errstate(all="ignore"):
        v = [((sR[i, 0] * X[:, 0] + sR[i, 1] * X[:, 1]) + sR[i, 2] * X[:, 2]) + t[i] for i in range(3)]
        if camera_type == PINHOLE:
            return np.stack([cam[0] * v[0] / v[2] + cam[2], cam[1] * v[1] / v[2] + cam[3]], 1).astype(F)
        x2y2 = v[0] * v[0] + v[1] * v[1]
        theta = np.arctan2(np.sqrt(x2y2.astype(np.float64)).astype(F).astype(np.float64), v[2].astype(np.float64)).astype(F)
        psi = np.arctan2(v[1].astype(np.float64), v[0].astype(np.float64)).astype(F)
        t2 = theta * theta
        t3 = theta * t2
        t5 = t3 * t2
        t7 = t5 * t2
        t9 = t7 * t2
        r = theta + cam[4] * t3 + cam[5] * t5 + cam[6] * t7 + cam[7] * t9
        return np.stack([cam[0] * r * np.cos(psi.astype(np.float64)).astype(F) + cam[2],
                         cam[1] * r * np.sin(psi.astype(np.float64)).astype(F) + cam[3]], 1).astype(F)


def errors(pb, T13):
    """err1, err2 [n] float32 of CheckInliers (:415-439)."""
    sR, t, sRinv, tinv = transforms(T13)
    X1, X2 = np.asarray(pb.x3dc1, F), np.asarray(pb.x3dc2, F)
    with np.errstate(all="ignore"):
        d1 = np.asarray(pb.p1im1, F) - project(pb.camera_type1, pb.camera1, sR, t, X2)
        d2 = project(pb.camera_type2, pb.camera2, sRinv, tinv, X1) - np.asarray(pb.p2im2, F)
        return (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]).astype(F), (d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]).astype(F)


def check_inliers(pb, T13):
    """The flags [n] and their count."""
    e1, e2 = errors(pb, T13)
    with np.errstate(all="ignore"):
        flags = (e1 < np.asarray(pb.max_error1, F)) & (e2 < np.asarray(pb.max_error2, F))
    return flags, int(flags.sum())


def threshold_margin(pb, T13):
    """How far the nearest error lies from its threshold, relative to the threshold (inf when an error is not finite)."""
    e1, e2 = errors(pb, T13)
    m1, m2 = np.asarray(pb.max_error1, np.float64), np.asarray(pb.max_error2, np.float64)
    with np.errstate(all="ignore"):
        d = np.concatenate([np.abs(e1.astype(np.float64) - m1) / m1, np.abs(e2.astype(np.float64) - m2) / m2])
    d = d[np.isfinite(d)]
    return float(d.min()) if d.size else float("inf")


def hypotheses(pb):
    """T [iterations, 13] of the problem's sets."""
    X1, X2 = np.asarray(pb.x3dc1, F), np.asarray(pb.x3dc2, F)
    return np.stack([compute_sim3(X1[s], X2[s], pb.fix_scale) for s in pb.sets]) if len(pb.sets) else np.zeros((0, 13), F)


def scan(count, min_inliers, best_in):
    """The records (count_k >= the running best), first_hit (the first record with count_k > min_inliers), the best at the end."""
    best, record, hit, last = best_in, [], -1, -1
    for k, c in enumerate(count):
        if c >= best:
            best, last = int(c), k
            record.append(k)
            if hit < 0 and c > min_inliers:
                hit = k
    return dict(record=record, first_hit=hit, best_iteration=last, best_count=best)


def solve(pb, T=None):
    """The whole pipeline: what osh_orb_sim3_ransac returns, with flags instead of mask words."""
    T = hypotheses(pb) if T is None else T
    flags = np.zeros((len(T), pb.n), bool)
    count = np.zeros(len(T), np.int32)
    for k, Tk in enumerate(T):
        flags[k], count[k] = check_inliers(pb, Tk)
    out = scan(count, pb.min_inliers, pb.best_inliers_in)
    out.update(count=count, T=T, flags=flags)
    return out


def max_iterations(N, probability, min_inliers, max_its):
    """mRansacMaxIts of SetRansacParameters (:123-147)."""
    with np.errstate(all="ignore"):
        eps = F(min_inliers) / F(N)
        if min_inliers == N:
            n_it = 1
        else:
            v = np.ceil(np.log(1 - probability) / np.log(1 - np.float64(eps) ** 3))
            n_it = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 - 1 else -2 ** 31
    return max(1, min(n_it, max_its))


class Replay:
    """The state of a Sim3Solver between iterate calls and the reference's loop (:167-210, :240-288) one iteration at a time over
    given per-iteration counts, transforms and flags."""

    def __init__(self, N, n1, indices1, min_inliers, max_its):
        self.N, self.n1, self.indices1, self.min_inliers, self.max_its = N, n1, np.asarray(indices1), min_inliers, max_its
        self.iterations, self.best_inliers = 0, 0
        self.best_flags, self.best_T = np.zeros(N, bool), None

    def reset(self, max_its):
        self.max_its, self.iterations = max_its, 0

    def iterate(self, n_iterations, count, T, flags, five=True):
        """count, T, flags are indexed by the solver's iteration number since the last reset."""
        out = dict(no_more=False, converged=False, inliers=np.zeros(self.n1, bool), n_inliers=0, T12=np.eye(4, dtype=F))
        if self.N < self.min_inliers or self.N < 3:
            out["no_more"] = True
            return out
        best_sim3 = np.eye(4, dtype=F)
        done = 0
        while self.iterations < self.max_its and done < n_iterations:
            done += 1
            k = self.iterations
            self.iterations += 1
            if count[k] >= self.best_inliers:
                self.best_flags, self.best_inliers, self.best_T = flags[k].copy(), int(count[k]), np.asarray(T[k], F)
                T12 = np.eye(4, dtype=F)
                T12[:3, :3] = self.best_T[12] * self.best_T[:9].reshape(3, 3)
                T12[:3, 3] = self.best_T[9:12]
                if count[k] > self.min_inliers:
                    out["n_inliers"] = int(count[k])
                    out["inliers"][self.indices1[flags[k]]] = True
                    out["converged"] = True
                    out["T12"] = T12
                    return out
                best_sim3 = T12
        if self.iterations >= self.max_its:
            out["no_more"] = True
        if five:
            out["T12"] = best_sim3
        return out
