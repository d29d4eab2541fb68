"""numpy restatement of the env adapter's foot-contact terms (include/hb.h: hb_env_feet) for the tests: every discrete decision in
float32 with its roundings made explicit, the terms in fp64, the record through steps and episode starts, the observation layout.
Test infrastructure only.

Semantics restated (F = body_contact[e][body][0:3], the read-out of the last physics substep; t = the env's float32 state time at the
evaluation, before any reset; "one rounding" = a single float32 multiply, add or subtract, never fused):
  in contact   n2 = (Fx*Fx + Fy*Fy) + Fz*Fz, each operation one rounding, in that order; c = n2 > thr*thr; the same test for feet,
               penalised bodies and terminal bodies
  air time     air_f = t - t_last[f] (one rounding); touchdown_f = c_f and not (mask bit f); the term is
               w_air_time * gate * sum_f (touchdown_f ? air_f - air_time_target : 0); gate = 1 when air_gate == 0, else
               (cx*cx + cy*cy > air_cmd_min*air_cmd_min) by the same float32 rule on the command in force during the step, or on
               hb_env_config.target_velocity when no commands are installed
  impact       w_force * sum_f max(sqrt(n2_f) - force_max, 0)
  stumble      s_f = c_f and (Fx*Fx + Fy*Fy) > (ratio*ratio) * (Fz*Fz), each product and sum one rounding; w_stumble once if any s_f
  collision    w_collision * the number of penalised bodies in contact
  termination  any terminal body in contact: terminated, OR-ed in before the terminal reward replaces the reward
  update       step evaluations only: t_last[f] = c_f ? t : t_last[f]; mask = the c_f bits.  Looking evaluations never write.
  episode      t_last[f] = the new state's time, all n_feet bits set
  row          [ base | prev_action | scan | foot_contact(n_feet) | command(3) ]; the flags are the mask after the evaluation's update
"""
import numpy as np

F = np.float32


def cfg_lists(C):
    """(foot, penalised, terminal) body ids of an HbEnvFeet (or anything with its fields)"""
    return ([int(C.foot_body[i]) for i in range(int(C.n_feet))], [int(C.penalised_body[i]) for i in range(int(C.n_penalised))],
            [int(C.terminal_body[i]) for i in range(int(C.n_terminal))])


def n2_parts(f3):
    """(n2, planar, normal) of one float32 force: (Fx*Fx + Fy*Fy) + Fz*Fz with every operation rounded once"""
    fx, fy, fz = F(f3[0]), F(f3[1]), F(f3[2])
    pl = F(F(fx * fx) + F(fy * fy))
    zz = F(fz * fz)
    return F(pl + zz), pl, zz


def in_contact(C, f3):
    thr = F(C.contact_threshold)
    return bool(n2_parts(f3)[0] > F(thr * thr))


def gate(C, cmd_xy):
    """the air-time gate on the planar command (or target velocity) in force during the step"""
    if not int(C.air_gate):
        return True
    cx, cy, lo = F(cmd_xy[0]), F(cmd_xy[1]), F(C.air_cmd_min)
    return bool(F(F(cx * cx) + F(cy * cy)) > F(lo * lo))


def start_record(C, time32):
    """the record of an episode that starts at float32 time time32: (t_last [n_feet] float32, mask)"""
    return np.full(int(C.n_feet), F(time32), dtype=np.float32), (1 << int(C.n_feet)) - 1


def evaluate(C, wrench, time32, t_last, mask, cmd_xy):
    """One evaluation of one env.  wrench: [nbody, >= 3] float32 (the read-out), time32: the state's float32 time, (t_last, mask): the
    record, cmd_xy: the planar command in force.  Returns a dict: the four terms (fp64, weighted) and their sum `reward`, `terminated`,
    `contact` (the c_f bits as a list), `touchdown`, `stumble`, `collisions`, and the record a STEP evaluation leaves: `t_last`, `mask`."""
    feet, pen, ter = cfg_lists(C)
    w = np.asarray(wrench, dtype=np.float32)
    t = F(time32)
    ratio = F(C.stumble_ratio)
    r2 = F(ratio * ratio)
    air_sum, force_sum, stumble = 0.0, 0.0, False
    c_bits, touch = [], []
    new_t = np.array(t_last, dtype=np.float32).copy()
    for f, body in enumerate(feet):
        n2, pl, zz = n2_parts(w[body])
        c = in_contact(C, w[body])
        td = c and not ((int(mask) >> f) & 1)
        if td:
            air_sum += float(F(t - F(t_last[f]))) - float(F(C.air_time_target))
        force_sum += max(float(np.sqrt(np.float64(n2))) - float(F(C.force_max)), 0.0)
        if c and bool(pl > F(r2 * zz)):
            stumble = True
        if c:
            new_t[f] = t
        c_bits.append(c)
        touch.append(td)
    ncol = sum(in_contact(C, w[b]) for b in pen)
    term = any(in_contact(C, w[b]) for b in ter)
    g = gate(C, cmd_xy)
    out = dict(air=float(F(C.w_air_time)) * air_sum * (1.0 if g else 0.0), force=float(F(C.w_force)) * force_sum,
               stumble_term=float(F(C.w_stumble)) if stumble else 0.0, collision=float(F(C.w_collision)) * ncol)
    out["reward"] = out["air"] + out["force"] + out["stumble_term"] + out["collision"]
    out.update(terminated=bool(term), contact=c_bits, touchdown=touch, stumble=stumble, collisions=int(ncol), gate=g,
               t_last=new_t, mask=sum(1 << f for f, c in enumerate(c_bits) if c))
    return out


class Record:
    """the records of n envs through episode starts and step evaluations"""

    def __init__(self, C, n, time32=None):
        self.C, self.n = C, int(n)
        self.start(np.zeros(self.n, dtype=np.float32) if time32 is None else time32)

    def start(self, time32, which=None):
        """an episode start (reset, configure, auto-reset) of the envs `which` (None: all) at their float32 times"""
        if which is None:
            self.t_last = np.zeros((self.n, int(self.C.n_feet)), dtype=np.float32)
            self.mask = np.zeros(self.n, dtype=np.int64)
            which = range(self.n)
        for e in which:
            self.t_last[e], self.mask[e] = start_record(self.C, np.asarray(time32, dtype=np.float32)[e])

    def step(self, wrench, time32, cmd_xy):
        """a step evaluation of every env: returns the list of evaluate() results and takes their records over"""
        res = [evaluate(self.C, wrench[e], time32[e], self.t_last[e], self.mask[e], cmd_xy[e]) for e in range(self.n)]
        for e, r in enumerate(res):
            self.t_last[e], self.mask[e] = r["t_last"], r["mask"]
        return res

    def look(self, wrench, time32, cmd_xy):
        """an evaluation that only looks (hb_get_obs, settle steps): the results, the record untouched"""
        return [evaluate(self.C, wrench[e], time32[e], self.t_last[e], self.mask[e], cmd_xy[e]) for e in range(self.n)]

    def contact(self):
        """[n, n_feet] uint8: the mask bits, what hb_env_get_feet and the observed flags carry"""
        return ((self.mask[:, None] >> np.arange(int(self.C.n_feet))[None, :]) & 1).astype(np.uint8)


def layout(nobs_base, nu, n_scan, prev_action, height_scan, n_feet_observed, cmd_observed):
    """the row [ base | prev_action | scan | foot_contact | command ] as slices; a part that is off is absent"""
    L = {"base": slice(0, nobs_base)}
    at = nobs_base
    if prev_action:
        L["prev_action"] = slice(at, at + nu); at += nu
    if height_scan:
        L["height_scan"] = slice(at, at + n_scan); at += n_scan
    if n_feet_observed:
        L["foot_contact"] = slice(at, at + n_feet_observed); at += n_feet_observed
    if cmd_observed:
        L["command"] = slice(at, at + 3); at += 3
    return L, at
