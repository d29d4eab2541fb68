"""numpy restatement of the env adapter's velocity commands (include/hb.h: hb_env_commands) for the tests: the draw with its float32
roundings made explicit, the resample rule on the state's float32 time, the heading frame, the two reward terms in fp64 on top of
env_ref.py's rewards, and the observation layout.  Test infrastructure only.

Semantics restated:
  storage   every env has a current command (cx, cy, cyaw) and the number k of draws made so far in its episode
  draw      draw k of episode ep of global env g: u_i = rng_uniform(seed, g, ep, k, RS_COMMAND = 40, i), i = 0..3; u_0 < zero_fraction gives
            (0, 0, 0); otherwise component c is lo_c + u_{c+1} * (hi_c - lo_c) in float32: a subtract, a multiply, an add, each rounded once
  when      draw 0 at every episode start (reset, auto-reset); inside an episode with resample_time > 0, after a step's reward and
            termination are formed, an env that did not reset and whose float32 time >= (float32)k * resample_time (a float32 product) makes
            draw k and sets k += 1; at most one draw per env step
  reward    a step is rewarded against the command in force during it (the one in obs[t]); the terminal observation carries that command;
            obs[t + 1] carries the new one.  Linear term w_hvel * scaled_exp(|v - (cx, cy)|^2), v = qvel[0:2] (frame 0) or the same vector in
            the root's heading frame (frame 1: the root's x axis flattened onto the world xy plane, unit (c, s), (1, 0) below a flattened
            length of 1e-6; v = (c vx + s vy, -s vx + c vy)); yaw term w_yaw * scaled_exp((wz - cyaw)^2), wz = the world z component of
            the root's angular velocity = R[2, :] . qvel[3:6] (the free joint's angular velocity is in the body frame); every other term,
            termination, truncation and the terminal reward as in env_ref.py; target_velocity is not read
  row       [ base | prev_action | scan | command(3) ], the command without noise or delay
"""
import numpy as np

import env_ref

RS_COMMAND = 40
F = np.float32
_LO = ("vx_min", "vy_min", "yaw_min")
_HI = ("vx_max", "vy_max", "yaw_max")


def draw(C, g, ep, k):
    """draw k of episode ep of global env g: float32 [3]"""
    u = [env_ref.rng_uniform(int(C.seed), int(g), int(ep), int(k), RS_COMMAND, i) for i in range(4)]
    if u[0] < F(C.zero_fraction):
        return np.zeros(3, dtype=np.float32)
    out = np.zeros(3, dtype=np.float32)
    for c in range(3):
        lo, hi = F(getattr(C, _LO[c])), F(getattr(C, _HI[c]))
        span = F(hi - lo)          # rounded once
        prod = F(u[c + 1] * span)  # rounded once
        out[c] = F(lo + prod)      # rounded once
    return out


def due(C, time32, k):
    """the resample rule: the state's float32 time against the float32 product (float32)k * resample_time"""
    rt = F(C.resample_time)
    return bool(rt > 0 and F(time32) >= F(F(k) * rt))


def root_matrix(qpos):
    q = np.asarray(qpos[3:7], dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def heading(qpos):
    """unit (c, s) of the root's x axis flattened onto the world xy plane; (1, 0) below a flattened length of 1e-6"""
    ax = root_matrix(qpos)[:, 0]
    n = np.hypot(ax[0], ax[1])
    return (1.0, 0.0) if n < 1e-6 else (ax[0] / n, ax[1] / n)


def planar_velocity(frame, qpos, qvel):
    vx, vy = float(qvel[0]), float(qvel[1])
    if frame == 0:
        return np.array([vx, vy])
    c, s = heading(qpos)
    return np.array([c * vx + s * vy, -s * vx + c * vy])


def yaw_rate(qpos, qvel):
    return float(root_matrix(qpos)[2] @ np.asarray(qvel[3:6], dtype=np.float64))


def linear_term(cfg, C, cmd, qpos, qvel):
    d = planar_velocity(int(C.frame), qpos, qvel) - np.asarray(cmd[:2], dtype=np.float64)
    return cfg.w_hvel * env_ref.scaled_exp(float(d @ d))


def yaw_term(C, cmd, qpos, qvel):
    return C.w_yaw * env_ref.scaled_exp((yaw_rate(qpos, qvel) - float(cmd[2])) ** 2)


def reward(cfg, C, cmd, time, qpos, qvel, joint_torques, prev_action, latest_action, self_collision):
    """(reward, terminated, truncated) of one env with commands installed: env_ref's reward of cfg.reward_kind without its own linear
    term, plus the two command terms; the terminal reward replaces everything"""
    base = env_ref.control_input_reward if cfg.reward_kind == 1 else env_ref.standup_reward
    c0 = type(cfg).from_buffer_copy(cfg)
    c0.w_hvel = 0.0
    r, term, trunc = base(c0, time, qpos, qvel, joint_torques, prev_action, latest_action, self_collision)
    if not term:
        r = r + linear_term(cfg, C, cmd, qpos, qvel) + yaw_term(C, cmd, qpos, qvel)
    return r, term, trunc


def rotate_state_z(qpos, qvel, angle):
    """the whole state turned by `angle` about the world z axis: root position, root orientation and the root's (world-frame) linear
    velocity; the root's angular velocity is in the body frame and every joint coordinate is relative, so they stay"""
    c, s = np.cos(angle), np.sin(angle)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    q, v = np.array(qpos, dtype=np.float64), np.array(qvel, dtype=np.float64)
    q[0:3] = Rz @ q[0:3]
    v[0:3] = Rz @ v[0:3]
    w0, x0, y0, z0 = q[3:7]
    cw, sz = np.cos(angle / 2), np.sin(angle / 2)  # (cw, 0, 0, sz) * q
    q[3:7] = [cw * w0 - sz * z0, cw * x0 - sz * y0, cw * y0 + sz * x0, cw * z0 + sz * w0]
    return q, v


def layout(nobs_base, nu, n_scan, prev_action, height_scan, observe):
    """the row [ base | prev_action | scan | command ] as slices; a part that is off is absent"""
    L = {"base": slice(0, nobs_base)}
    at = nobs_base
    if prev_action:
        L["prev_action"] = slice(at, at + nu); at += nu
    if height_scan:
        L["height_scan"] = slice(at, at + n_scan); at += n_scan
    if observe:
        L["command"] = slice(at, at + 3); at += 3
    return L, at


class Schedule:
    """the commands of n envs (global indices env_offset + e) through resets and steps"""

    def __init__(self, C, n, env_offset=0):
        self.C, self.n, self.off = C, int(n), int(env_offset)
        self.reset()

    def reset(self, episodes=None):
        """draw 0 of the episodes the envs start in (all zero after a plain reset)"""
        self.ep = np.zeros(self.n, dtype=np.int64) if episodes is None else np.array(episodes, dtype=np.int64)
        self.k = np.ones(self.n, dtype=np.int64)
        self.cmd = np.stack([draw(self.C, self.off + e, self.ep[e], 0) for e in range(self.n)])
        return self.cmd.copy()

    def set(self, cmd, mask=None):
        """the override: the chosen envs' commands, their draw counters untouched"""
        m = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.cmd[m] = np.asarray(cmd, dtype=np.float32)[m]

    def step(self, time32, ended):
        """one env step whose post-step float32 times are time32 and whose envs `ended` were reset in place: returns the commands the
        step was rewarded against (those of the terminal rows); self.cmd is then what obs[t + 1] carries"""
        old = self.cmd.copy()
        for e in range(self.n):
            if ended[e]:
                self.ep[e] += 1
                self.cmd[e] = draw(self.C, self.off + e, self.ep[e], 0)
                self.k[e] = 1
            elif due(self.C, time32[e], self.k[e]):
                self.cmd[e] = draw(self.C, self.off + e, self.ep[e], self.k[e])
                self.k[e] += 1
        return old
