"""fp64 restatement of inverse dynamics (include/hb.h: hb_inverse; mj_inverse [recall]) on the oracle's forward() arrays.

TEST INFRASTRUCTURE, like env_ref.py: the product package never imports it.

    qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - J' f,   f_i = -D_i jar_i if jar_i = J_i qacc - aref_i < 0, else 0
    discrete (mjENBL_INVDISCRETE): qacc is (qvel' - qvel) / h of the Euler step with implicit damping, and is first turned into
    the continuous acceleration qacc + M^-1 (h diag(damping) qacc)
"""
import numpy as np

DSBL_EULERDAMP = 1 << 14


def inverse_terms(o, qacc, discrete=False):
    """o: an oracle_lib.Oracle whose forward() has run at the state of interest; qacc [nv] -> the terms of qfrc_inverse (fp64):
    M qacc, qfrc_bias, qfrc_passive, J' f, and the number of active rows"""
    nv, ne = o.nv, o.nefc
    M = o.dense_M()
    qacc = np.asarray(qacc, dtype=np.float64)
    if discrete:
        damping = o.marr("dof_damping")
        if not (o.opt("disableflags") & DSBL_EULERDAMP) and (damping > 0).any():
            qacc = qacc + np.linalg.solve(M, o.opt("timestep") * damping * qacc)
    qfc, active = np.zeros(nv), 0
    if ne:
        J = o.efc_J.reshape(ne, nv)
        jar = J @ qacc - o.efc_aref
        f = np.where(jar < 0.0, -jar / o.efc_R, 0.0)
        qfc, active = J.T @ f, int((jar < 0.0).sum())
    return dict(Mqacc=M @ qacc, bias=o.qfrc_bias.copy(), passive=o.qfrc_passive.copy(), constraint=qfc, active=active)


def inverse_ref(o, qacc, discrete=False):
    """qfrc_inverse [nv] (fp64) at the oracle's current forward() state"""
    t = inverse_terms(o, qacc, discrete)
    return t["Mqacc"] + t["bias"] - t["passive"] - t["constraint"]


def force_scale(t):
    """the largest entry of any term of qfrc_inverse (at least 1): what fp32 rounding of the sum is relative to"""
    return max(1.0, *(float(np.abs(t[k]).max()) for k in ("Mqacc", "bias", "passive", "constraint")))


def forward_at(o, qpos, qvel, ctrl=None):
    """The oracle's mj_forward at (qpos, qvel[, ctrl]), xfrc_applied and qfrc_applied zero."""
    o.reset()
    o.qpos[:] = qpos
    o.qvel[:] = qvel
    if ctrl is not None:
        o.ctrl[:] = ctrl
    o.forward()
