"""Independent numpy rigid-body dynamics (Jacobian / Lagrangian formulation).

Two uses, neither on the product's step path:

1. ``invweight0`` restates the part of MuJoCo's ``mj_setConst`` ([UPSTREAM] engine_setconst.c, called
   by the reference at /root/reference mujoco_ros/src/callbacks.cpp:254,582 and implicitly by
   ``mj_loadXML``) that fills ``dof_invweight0`` / ``body_invweight0`` -- model-compile-time
   constants the constraint stage reads.
2. The tests use ``mass_matrix`` / ``bias_lagrange`` / ``bias_newton_euler`` / ``step_euler`` as a
   *differently derived* check of the C oracle's and the HIP kernels' CRB, RNE and Euler step
   (SURVEY.md §8c substitute oracle (ii)): M from body Jacobians, bias from finite-differenced
   Lagrangian terms (hinge / slide models) and from Newton's and Euler's equations projected through
   finite-differenced Jacobians (hinge, slide, ball and free joints, any number of joints per body,
   a ball being the last rotational joint of its body).  On hinge / slide models the two biases are
   independent derivations of one quantity.  Nothing here shares code or algorithm with oracle/ or csrc/.
"""
from __future__ import annotations

import numpy as np

JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3


def _quat_mul(a, b):
    return np.array([
        a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
        a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
        a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
        a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _quat2mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _axis_angle_quat(axis, angle):
    return np.concatenate([[np.cos(angle / 2)], np.asarray(axis) * np.sin(angle / 2)])


def kinematics(m, qpos):
    """World poses of bodies, inertial frames, joint anchors/axes for generalized position qpos."""
    nb, nj = m["nbody"], m["njnt"]
    xpos = np.zeros((nb, 3))
    xquat = np.tile(np.array([1.0, 0, 0, 0]), (nb, 1))
    xanchor = np.zeros((nj, 3))
    xaxis = np.zeros((nj, 3))
    for b in range(1, nb):
        p = m["body_parentid"][b]
        ja, jn = m["body_jntadr"][b], m["body_jntnum"][b]
        if jn == 1 and m["jnt_type"][ja] == JNT_FREE:
            qa = m["jnt_qposadr"][ja]
            pos = qpos[qa:qa + 3].copy()
            q = qpos[qa + 3:qa + 7] / np.linalg.norm(qpos[qa + 3:qa + 7])
            xanchor[ja] = pos
            xaxis[ja] = m["jnt_axis"][ja]
        else:
            Rp = _quat2mat(xquat[p])
            pos = xpos[p] + Rp @ m["body_pos"][b]
            q = _quat_mul(xquat[p], m["body_quat"][b])
            for j in range(ja, ja + jn):
                qa = m["jnt_qposadr"][j]
                R = _quat2mat(q)
                xaxis[j] = R @ m["jnt_axis"][j]
                xanchor[j] = pos + R @ m["jnt_pos"][j]
                t = m["jnt_type"][j]
                if t == JNT_SLIDE:
                    pos = pos + xaxis[j] * (qpos[qa] - m["qpos0"][qa])
                else:
                    if t == JNT_BALL:
                        ql = qpos[qa:qa + 4] / np.linalg.norm(qpos[qa:qa + 4])
                    else:
                        ql = _axis_angle_quat(m["jnt_axis"][j], qpos[qa] - m["qpos0"][qa])
                    q = _quat_mul(q, ql)
                    pos = xanchor[j] - _quat2mat(q) @ m["jnt_pos"][j]
        xpos[b] = pos
        xquat[b] = q / np.linalg.norm(q)
    xmat = np.array([_quat2mat(q) for q in xquat])
    xipos = np.array([xpos[b] + xmat[b] @ m["body_ipos"][b] for b in range(nb)])
    ximat = np.array([xmat[b] @ _quat2mat(m["body_iquat"][b]) for b in range(nb)])
    return dict(xpos=xpos, xquat=xquat, xmat=xmat, xipos=xipos, ximat=ximat, xanchor=xanchor, xaxis=xaxis)


def jac_point(m, kin, body, point):
    """Translational (at ``point``, fixed to ``body``) and rotational Jacobians, 3 x nv each."""
    nv = m["nv"]
    jp = np.zeros((3, nv))
    jr = np.zeros((3, nv))
    b = body
    while b > 0:
        ja, jn = m["body_jntadr"][b], m["body_jntnum"][b]
        for j in range(ja, ja + jn):
            d = m["jnt_dofadr"][j]
            t = m["jnt_type"][j]
            if t == JNT_HINGE:
                ax = kin["xaxis"][j]
                jr[:, d] = ax
                jp[:, d] = np.cross(ax, point - kin["xanchor"][j])
            elif t == JNT_SLIDE:
                jp[:, d] = kin["xaxis"][j]
            elif t == JNT_BALL:
                for k in range(3):
                    ax = kin["xmat"][b][:, k]
                    jr[:, d + k] = ax
                    jp[:, d + k] = np.cross(ax, point - kin["xanchor"][j])
            else:  # free
                for k in range(3):
                    jp[k, d + k] = 1.0
                    ax = kin["xmat"][b][:, k]
                    jr[:, d + 3 + k] = ax
                    jp[:, d + 3 + k] = np.cross(ax, point - kin["xpos"][b])
        b = m["body_parentid"][b]
    return jp, jr


def mass_matrix(m, qpos, kin=None):
    """Dense joint-space inertia  M = sum_b m_b Jp'Jp + Jr' (R I R') Jr  + diag(armature)."""
    kin = kin or kinematics(m, qpos)
    nv = m["nv"]
    M = np.diag(np.asarray(m["dof_armature"], dtype=np.float64)).copy() if nv else np.zeros((0, 0))
    for b in range(1, m["nbody"]):
        if m["body_mass"][b] == 0 and not np.any(m["body_inertia"][b]):
            continue
        jp, jr = jac_point(m, kin, b, kin["xipos"][b])
        Iw = kin["ximat"][b] @ np.diag(m["body_inertia"][b]) @ kin["ximat"][b].T
        M += m["body_mass"][b] * jp.T @ jp + jr.T @ Iw @ jr
    return M


def potential(m, qpos):
    kin = kinematics(m, qpos)
    g = np.asarray(m["gravity"], dtype=np.float64)
    return -sum(m["body_mass"][b] * np.dot(g, kin["xipos"][b]) for b in range(1, m["nbody"]))


def gravcomp_force(m, qpos):
    """Generalized force of MuJoCo's body gravity compensation (mj_passive, body_gravcomp), from its definition:

        sum_b  Jp_b' (-g m_b gc_b),      Jp_b the translational Jacobian of body b at its centre of mass,

    zero when gravity is zero.  (The disable flags are the caller's business: this is the term itself.)"""
    qpos = np.asarray(qpos, dtype=np.float64)
    kin = kinematics(m, qpos)
    g = np.asarray(m["gravity"], dtype=np.float64)
    gc = np.asarray(m["body_gravcomp"], dtype=np.float64) if "body_gravcomp" in m else np.zeros(m["nbody"])
    out = np.zeros(m["nv"])
    for b in range(1, m["nbody"]):
        if gc[b] != 0:
            jp, _ = jac_point(m, kin, b, kin["xipos"][b])
            out += jp.T @ (-g * m["body_mass"][b] * gc[b])
    return out


def bias_lagrange(m, qpos, qvel, eps=1e-6):
    """Coriolis + centrifugal + gravity generalized force c(q,v) such that  M a + c = tau,
    from the Lagrangian (central finite differences of M(q) and V(q)).  Hinge/slide joints only
    (qpos is then a vector space and d/dt qpos = qvel)."""
    if np.any(np.asarray(m["jnt_type"]) < JNT_SLIDE):
        raise ValueError("bias_lagrange supports hinge/slide models only")
    n = m["nv"]
    dM = np.zeros((n, n, n))  # dM[k] = dM/dq_k
    dV = np.zeros(n)
    for k in range(n):
        e = np.zeros(n)
        e[k] = eps
        dM[k] = (mass_matrix(m, qpos + e) - mass_matrix(m, qpos - e)) / (2 * eps)
        dV[k] = (potential(m, qpos + e) - potential(m, qpos - e)) / (2 * eps)
    Mdot = np.tensordot(qvel, dM, axes=(0, 0))
    c = Mdot @ qvel - 0.5 * np.array([qvel @ dM[k] @ qvel for k in range(n)]) + dV
    return c


def _quat_exp(w, t):
    """Unit quaternion of the rotation by angle t |w| about w."""
    w = np.asarray(w, dtype=np.float64)
    n = np.linalg.norm(w)
    if n == 0:
        return np.array([1.0, 0, 0, 0])
    return np.concatenate([[np.cos(0.5 * t * n)], w / n * np.sin(0.5 * t * n)])


def integrate_pos(m, qpos, qvel, t):
    """qpos moved for time t along constant qvel, on the configuration manifold: hinge / slide add, a ball joint's
    quaternion is right-multiplied by exp(t w) (w in the body's frame), a free joint moves pos by t v and its quaternion
    as a ball's."""
    q = np.array(qpos, dtype=np.float64)
    v = np.asarray(qvel, dtype=np.float64)
    for j in range(m["njnt"]):
        ty, qa, da = m["jnt_type"][j], m["jnt_qposadr"][j], m["jnt_dofadr"][j]
        if ty == JNT_FREE:
            q[qa:qa + 3] += t * v[da:da + 3]
            q[qa + 3:qa + 7] = _quat_mul(q[qa + 3:qa + 7], _quat_exp(v[da + 3:da + 6], t))
        elif ty == JNT_BALL:
            q[qa:qa + 4] = _quat_mul(q[qa:qa + 4], _quat_exp(v[da:da + 3], t))
        else:
            q[qa] += t * v[da]
    return q


def _check_ball_last(m):
    for b in range(1, m["nbody"]):
        ja, jn = m["body_jntadr"][b], m["body_jntnum"][b]
        for j in range(ja, ja + jn):
            if m["jnt_type"][j] == JNT_BALL and any(m["jnt_type"][k] != JNT_SLIDE for k in range(j + 1, ja + jn)):
                raise ValueError("bias_newton_euler needs a ball joint to be the last rotational joint of its body")


def bias_newton_euler(m, qpos, qvel, eps=1e-6):
    """Coriolis + centrifugal + gravity generalized force c(q,v) such that  M a + c = tau, as the body-by-body projection of
    Newton's and Euler's equations at zero joint acceleration:

        c = sum_b  Jp_b' m_b (dJp_b/dt v - g)  +  Jr_b' (I_b dJr_b/dt v + w_b x I_b w_b),      w_b = Jr_b v,

    with Jp_b at the body's centre of mass, I_b its inertia in world axes, and dJ/dt a central difference of ``jac_point``
    along ``integrate_pos`` (the exact flow of constant qvel).  Hinge, slide, ball and free joints, any number of joints
    per body.

    The ball-last condition: ``jac_point`` (as MuJoCo's cdof) gives a ball joint's three columns in the body's FINAL
    frame.  That is d/dt of the kinematics along ``integrate_pos`` only if no rotation follows the ball on the same body,
    so a ball joint must be the last rotational joint of its body (slides may follow).  ValueError otherwise."""
    _check_ball_last(m)
    qpos = np.asarray(qpos, dtype=np.float64)
    v = np.asarray(qvel, dtype=np.float64)

    def jacs(q):
        kin = kinematics(m, q)
        return kin, [jac_point(m, kin, b, kin["xipos"][b]) for b in range(m["nbody"])]

    kin, J = jacs(qpos)
    _, Jf = jacs(integrate_pos(m, qpos, v, eps))
    _, Jb = jacs(integrate_pos(m, qpos, v, -eps))
    g = np.asarray(m["gravity"], dtype=np.float64)
    c = np.zeros(m["nv"])
    for b in range(1, m["nbody"]):
        jp, jr = J[b]
        djp = (Jf[b][0] - Jb[b][0]) / (2 * eps)
        djr = (Jf[b][1] - Jb[b][1]) / (2 * eps)
        Iw = kin["ximat"][b] @ np.diag(m["body_inertia"][b]) @ kin["ximat"][b].T
        w = jr @ v
        c += m["body_mass"][b] * jp.T @ (djp @ v - g) + jr.T @ (Iw @ (djr @ v) + np.cross(w, Iw @ w))
    return c


def step_euler(m, qpos, qvel, qfrc):
    """One semi-implicit Euler step with implicit joint damping of a model WITHOUT constraints:

        v' = v + h (M + h B)^-1 (qfrc - c - B v),     q' = integrate_pos(q, v', h),      B = diag(dof_damping),

    where qfrc is every generalized force other than bias and joint damping (springs, actuators, applied).
    Returns (q', v', qacc_smooth) with  M qacc_smooth = qfrc - c - B v."""
    qpos = np.asarray(qpos, dtype=np.float64)
    v = np.asarray(qvel, dtype=np.float64)
    h = float(np.asarray(m["timestep"]).ravel()[0])
    M = mass_matrix(m, qpos)
    B = np.diag(np.asarray(m["dof_damping"], dtype=np.float64))
    f = np.asarray(qfrc, dtype=np.float64) - bias_newton_euler(m, qpos, v) - B @ v
    vn = v + h * np.linalg.solve(M + h * B, f)
    return integrate_pos(m, qpos, vn, h), vn, np.linalg.solve(M, f)


def invweight0(m):
    """dof_invweight0[nv], body_invweight0[nbody,2], stat.meaninertia at qpos0 (restates mj_setConst's set0)."""
    nv, nb = m["nv"], m["nbody"]
    dof_inv = np.zeros(nv)
    body_inv = np.zeros((nb, 2))
    if nv == 0:
        return dof_inv, body_inv, 1.0
    kin = kinematics(m, np.asarray(m["qpos0"], dtype=np.float64))
    M = mass_matrix(m, m["qpos0"], kin)
    Minv = np.linalg.inv(M)
    for b in range(1, nb):
        if m["body_weldid"][b] == 0:
            continue
        jp, jr = jac_point(m, kin, b, kin["xipos"][b])
        A = np.vstack([jp, jr]) @ Minv @ np.vstack([jp, jr]).T
        body_inv[b, 0] = (A[0, 0] + A[1, 1] + A[2, 2]) / 3
        body_inv[b, 1] = (A[3, 3] + A[4, 4] + A[5, 5]) / 3
    for j in range(m["njnt"]):
        d = m["jnt_dofadr"][j]
        t = m["jnt_type"][j]
        if t in (JNT_HINGE, JNT_SLIDE):
            dof_inv[d] = Minv[d, d]
        elif t == JNT_BALL:
            dof_inv[d:d + 3] = np.trace(Minv[d:d + 3, d:d + 3]) / 3
        else:
            dof_inv[d:d + 3] = np.trace(Minv[d:d + 3, d:d + 3]) / 3
            dof_inv[d + 3:d + 6] = np.trace(Minv[d + 3:d + 6, d + 3:d + 6]) / 3
    return dof_inv, body_inv, float(np.mean(np.diag(M)))
