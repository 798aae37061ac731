"""Social-force pedestrian policy (no counterpart in the reference; the model is defined in include/mcn.h).

For the env's own humans this class is a parameter carrier, like ORCA: VecCrowdSim reads strength / range /
relaxation_rate from it and the model runs fused inside env_step.hip (mcn_env_step_sf).  `predict()` evaluates the same
formula on the host in float64, operation for operation, for agents outside that kernel (E = 1 API completeness).
"""
import math

from .policy import Policy
from ..utils.action import ActionXY


class SocialForce(Policy):
    def __init__(self):
        super().__init__()
        self.name = "SocialForce"
        self.trainable = False
        self.multiagent_training = None
        self.kinematics = "holonomic"
        self.strength = 4.0             # A, m/s^2
        self.range = 0.2                # B, m
        self.relaxation_rate = 2.0      # k, 1/s (relaxation time 0.5 s)

    def configure(self, config):
        """Optional [social_force] section of env.config."""
        if config is not None and config.has_section("social_force"):
            self.strength = config.getfloat("social_force", "strength", fallback=self.strength)
            self.range = config.getfloat("social_force", "range", fallback=self.range)
            self.relaxation_rate = config.getfloat("social_force", "relaxation_rate", fallback=self.relaxation_rate)
        if not (math.isfinite(self.strength) and math.isfinite(self.range) and math.isfinite(self.relaxation_rate)
                and self.strength >= 0 and self.range > 0 and self.relaxation_rate >= 0):
            raise ValueError("[social_force] needs finite strength >= 0, range > 0, relaxation_rate >= 0")

    def set_phase(self, phase):
        return

    def predict(self, state):
        """state.human_states are the others, in the order given (a visible robot is simply one of them)."""
        me = state.self_state
        A, B, k, dt, s = self.strength, self.range, self.relaxation_rate, self.time_step, me.v_pref
        ex, ey = me.gx - me.px, me.gy - me.py
        d = math.sqrt(ex * ex + ey * ey)
        if d > s:
            ex, ey = ex / d * s, ey / d * s
        ax, ay = k * (ex - me.vx), k * (ey - me.vy)
        for o in state.human_states:
            dx, dy = me.px - o.px, me.py - o.py
            dist = math.sqrt(dx * dx + dy * dy)
            if dist > 0:
                m = A * math.exp((me.radius + o.radius - dist) / B)
                ax = ax + m * (dx / dist)
                ay = ay + m * (dy / dist)
        wx, wy = me.vx + ax * dt, me.vy + ay * dt
        n = math.sqrt(wx * wx + wy * wy)
        if n > s:
            wx, wy = wx / n * s, wy / n * s
        self.last_state = state
        return ActionXY(wx, wy)
