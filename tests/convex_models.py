"""MJCF pieces of the convex collision tests (tests/test_oracle_convex.py, tests/test_gpu_convex.py, tests/test_gpu_staged.py): a cube and
a rounded hull as <mesh> assets, a height-field floor with a body on it, a cube hull on a plane.

TEST INFRASTRUCTURE, pure numpy: the product package never imports this module.
"""
import numpy as np

CUBE = np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)])
CUBE_MESH = '<mesh name="cube" vertex="%s"/>' % " ".join("%g" % (0.1 * v) for v in CUBE.reshape(-1))


def _ball_points(n=300, r=0.05):
    k = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * k / n)
    th = np.pi * (1 + 5 ** 0.5) * k
    return r * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)


BALL_MESH = '<mesh name="ball" vertex="%s"/>' % " ".join("%.9g" % v for v in _ball_points().reshape(-1))


def hfield_xml(elev, body, nrow=4, ncol=4, size="2 2 1 0.5", extra=""):
    return ('<mujoco><option timestep="0.002"/><asset><hfield name="h" nrow="%d" ncol="%d" size="%s" elevation="%s"/>%s</asset>'
            '<worldbody><geom name="floor" type="hfield" hfield="h" condim="6" friction="1.5"/>%s</worldbody></mujoco>'
            % (nrow, ncol, size, " ".join("%.17g" % v for v in np.asarray(elev).reshape(-1)), extra, body))


# ---- mjc_PlaneConvex: mesh hulls on a PLANE floor (the reference's green_screen_world.xml:30 and empty_world.xml:24 put the robot's
# meshes on one; rl/generate_policy_videos.py builds CPUEnv on it)
PLANE_CUBE_XML = ('<mujoco><option timestep="0.002"/><asset>%s</asset><worldbody><geom name="floor" type="plane" pos="0 0 0" size="0 0 .05" condim="3"/>'
                  '<body pos="%s" %s><freejoint/><inertial pos="0 0 0" mass="0.5" diaginertia="0.001 0.001 0.001"/><geom type="mesh" mesh="cube" condim="%d"/></body>'
                  '</worldbody></mujoco>')
