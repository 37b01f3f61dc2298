"""Activation states (mjData.act: dyntype integrator / filter, <intvelocity>, <cylinder>) in the lane = env kernel (csrc/mjb_lane_env_kernel.h,
`if constexpr (T::NA > 0)`): act in the lane's registers for the launch, act_dot from the clamped ctrl, the force from the current act, one advance per
step -- against the CPU oracle and against the generic 16-lanes-per-env kernel running the same batch.

Bounds, those tests/test_gpu_lane_env_xfrc.py holds the same comparisons to: one step against the oracle 1e-11 (1 + |x|); rollouts of 60 steps or fewer,
and the lane = env kernel against the generic one, 1e-9 (1 + |x|); energy rtol 1e-7; bit equality where a test says so.  70 envs = one full wavefront and
a 6-lane tail; envs 0, 63, 64, 69 go against the oracle where not every env does.  Models, states and the oracle's rollouts: tests/test_lane_env_act.py."""
import numpy as np
import pytest

from mujoco_ros_pkgs_amd import mjcf
from test_gpu_lane_env_params import apply, draw, twin_model
from test_lane_env_act import CHECK, MODELS, NENV, NOISE, ROLLOUT, oracle_env, reference_rollout, states

pytestmark = pytest.mark.gpu

FIELDS = ("qpos", "qvel", "qacc", "act", "sensordata")
EVERY = FIELDS + ("energy", "time", "ctrl")
DSBL_CLAMPCTRL, DSBL_ACTUATION = 1 << 7, 1 << 10


def _err(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want)))) if want.size else 0.0


def _close(got, want, tol, what):
    err = _err(got, want)
    print(f"{what}: {err:.3e} (bound {tol:.0e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.0e}"


def make(engine, cm, S, mode=1, noise=None, ctrl=True):
    qpos, qvel, c, act = S
    b = engine.Batch(cm, qpos.shape[0])
    b.set_lane_env(mode)
    b.set("qpos", qpos)
    b.set("qvel", qvel)
    b.set("act", act)
    if ctrl:
        b.set("ctrl", c)
    if noise:
        b.set_ctrl_noise(*noise)
    return b


def ran(b, lane):
    assert bool(b.lane_env_info()[1]) == lane, f"lane = env kernel used: {b.lane_env_info()[1]}, expected {lane} ({b.lane_env_error()})"
    if lane:
        assert b.lane_env_last_form() == 0


def snapshot(b, fields=EVERY):
    return {f: b.get(f) for f in fields}


def against_oracle(po, model, got, S, K, tol, envs, what, noise=None, xfrc=None, models=None):
    qpos, qvel, ctrl, act = S
    worst = 0.0
    for e in envs:
        d = oracle_env(po, models[e] if models else model, qpos[e], qvel[e], None if noise else ctrl[e], act[e], K, noise, e, None if xfrc is None else xfrc[e])
        for f in FIELDS:
            err = _err(got[f][e], d.field(f))
            worst = max(worst, err)
            assert err <= tol, f"{what} env {e}, {K} steps: {f} {err:.2e} > {tol:.0e}"
        if int(model["enableflags"]) & 2:
            assert np.allclose(got["energy"][e], d.energy, rtol=1e-7, atol=1e-8), f"{what} env {e}: energy {got['energy'][e]} vs {d.energy}"
    print(f"{what} K={K}: worst error against the oracle over {len(list(envs))} envs {worst:.2e} (bound {tol:.0e})")


def against_generic(got, ref, tol, what, fields=EVERY):
    for f in fields:
        _close(got[f], ref[f], tol, f"{what}: {f} against the generic kernel")


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel choice
def test_kernel_choice(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    for which in ("A", "B"):
        model = MODELS[which](energy=True)
        cm = engine.CompiledModel(model)
        S = states(which, model)
        b = make(engine, cm, S)
        assert b.lane_env_info()[0] == -2
        for form in (-1, 3):  # (whatever form is asked for: one wavefront per 64 envs)
            engine.binding.load_library().mjb_lane_env_set_form(form)
            try:
                b.step(1)
            finally:
                engine.binding.load_library().mjb_lane_env_set_form(-1)
            ran(b, True)
        b.close()
        auto = make(engine, cm, S, mode=-1)  # the automatic mode: not at 70 envs ...
        auto.step(1)
        ran(auto, False)
        auto.close()
    model = MODELS["A"](energy=True)
    cm = engine.CompiledModel(model)
    big = make(engine, cm, states("A", model, 4096), mode=-1)  # ... and at 4096
    big.step(1)
    ran(big, True)
    assert np.all(np.isfinite(big.get("act"))) and np.all(np.isfinite(big.get("qpos")))
    big.close()
    # with a hwsim stage: no build of the kernel has both -- the generic kernel, bit-equal to a mode-0 batch
    S = states("A", model)
    eff = np.random.default_rng(8).uniform(-2, 2, (NENV, 1))
    out = []
    for mode in (1, 0):
        b = make(engine, cm, S, mode=mode)
        b.set_lane_env_hwsim(True)
        b.hwsim_configure([dict(joint=1, method="effort")])
        b.hwsim_set_command("effort", eff)
        b.step(5)
        ran(b, False)
        assert b.lane_env_info()[0] == -2  # (not marked unavailable: without the stage the batch would run the kernel)
        out.append(snapshot(b))
        b.close()
    for f in EVERY:
        assert np.array_equal(out[0][f], out[1][f]), f


# ------------------------------------------------------------------------------------------------------- 2. one step against the oracle
@pytest.mark.parametrize("which", ["A", "B"])
def test_one_step(oracle_built, which):
    from mujoco_ros_pkgs_amd import engine
    model = MODELS[which](energy=True)
    cm = engine.CompiledModel(model)
    S = states(which, model)
    b = make(engine, cm, S)
    b.step(1)
    ran(b, True)
    got = snapshot(b)
    b.close()
    against_oracle(oracle_built, model, got, S, 1, 1e-11, range(NENV), f"model {which}")
    assert _err(got["act"], S[3]) > 1e-4  # (act did advance)
    g = make(engine, cm, S, mode=0)
    g.step(1)
    ran(g, False)
    against_generic(got, snapshot(g), 1e-9, f"model {which}")
    g.close()


# ---------------------------------------------------------------------- 3. - 5. rollouts, launch splits, hand-overs to the generic kernel
@pytest.mark.parametrize("noisy", [True, False], ids=["ctrl_noise", "drawn_ctrl"])
@pytest.mark.parametrize("which", ["A", "B"])
def test_rollout(oracle_built, which, noisy):
    """60 steps, under the ctrl-noise injector (every env's tight integrator sits at an actrange bound within a few steps) and under the drawn ctrl (the
    oracle's rollout meets a bound in at least 8 envs and never in at least 8 others, tests/test_lane_env_act.py): the four envs against the oracle and
    every env against the generic kernel, act included."""
    from mujoco_ros_pkgs_amd import engine
    model = MODELS[which](energy=True)
    cm = engine.CompiledModel(model)
    S = states(which, model)
    ref, hit = reference_rollout(which, noisy)
    assert hit.sum() >= 8 and (noisy or (~hit).sum() >= 8)
    res = []
    for mode in (1, 0):
        b = make(engine, cm, S, mode=mode, noise=NOISE if noisy else None, ctrl=not noisy)
        b.step(ROLLOUT)
        ran(b, mode == 1)
        res.append(snapshot(b))
        b.close()
    worst = 0.0
    for e in CHECK:
        for f in FIELDS:
            err = _err(res[0][f][e], ref[e][f])
            worst = max(worst, err)
            assert err <= 1e-9, f"model {which} env {e}, {ROLLOUT} steps: {f} {err:.2e} > 1e-09"
    print(f"model {which} K={ROLLOUT}: worst error against the oracle over {len(CHECK)} envs {worst:.2e} (bound 1e-09)")
    against_generic(res[0], res[1], 1e-9, f"model {which} {ROLLOUT} steps")
    lim = [i for i in range(model["nu"]) if model["actuator_actlimited"][i]]
    rngs = np.asarray(model["actuator_actrange"], float).reshape(-1, 2)
    for i in lim:
        a = res[0]["act"][:, int(model["actuator_actadr"][i])]
        assert np.all((a >= rngs[i, 0]) & (a <= rngs[i, 1]))


@pytest.mark.parametrize("which", ["A", "B"])
def test_launch_splits_and_interleaving(oracle_built, which):
    """20 steps are 7 + 13 steps bit for bit on every field, act included (act crosses DevState::act between launches); 10 lane = env steps, 10 generic
    steps, 10 lane = env steps against 30 generic steps -- the 10 in the middle as one fused launch, and as ten step1 / step2 pairs on the full frame."""
    from mujoco_ros_pkgs_amd import engine
    model = MODELS[which](energy=True)
    cm = engine.CompiledModel(model)
    S = states(which, model)
    res = {}
    for name, plan in (("whole", [(1, 20)]), ("split", [(1, 7), (1, 13)]), ("mixed", [(1, 10), (0, 10), (1, 10)]), ("halves", [(1, 10), ("step1 / step2", 10), (1, 10)]),
                       ("generic", [(0, 30)])):
        b = make(engine, cm, S, noise=NOISE, ctrl=False)
        for mode, k in plan:
            if mode == "step1 / step2":
                for _ in range(k):
                    b.step1()
                    b.step2()
                continue
            b.set_lane_env(mode)
            b.step(k)
            ran(b, mode == 1)
        res[name] = snapshot(b)
        b.close()
    for f in EVERY:
        assert np.array_equal(res["whole"][f], res["split"][f]), f"splitting a launch changed {f}"
    against_generic(res["mixed"], res["generic"], 1e-9, f"model {which}, a generic launch in the middle")
    against_generic(res["halves"], res["generic"], 1e-9, f"model {which}, step1 / step2 pairs in the middle", FIELDS + ("time",))
    assert _err(res["mixed"]["act"], S[3]) > 1e-4


# ---------------------------------------------------------------------------------------------------------------------------- 6. resets
def test_resets_inside_a_launch(oracle_built):
    """Env 5's qvel trips mj_checkVel at the first step; env 20's ctrl on the <cylinder> (no ctrlrange, no forcerange) winds its act up until the force
    trips mj_checkAcc at the second.  mj_resetData zeroes act: both envs end the launch with act == 0 and the generic kernel's and the oracle's warning
    counters, their later steps match both, and the other lanes of the wavefront are bit-equal to a batch without the two bad envs."""
    from mujoco_ros_pkgs_amd import engine
    po = oracle_built
    model = MODELS["A"](energy=True)
    cm = engine.CompiledModel(model)
    qpos, qvel, ctrl, act = states("A", model)
    clean = (qpos.copy(), qvel.copy(), ctrl.copy(), act)
    qvel[5, 1] = 1e12
    ctrl[20, 4] = 1e14
    S = (qpos, qvel, ctrl, act)
    lane, gen, tidy = make(engine, cm, S), make(engine, cm, S, mode=0), make(engine, cm, clean)
    for b in (lane, gen, tidy):
        b.step(3)
    ran(lane, True)
    ran(gen, False)
    ran(tidy, True)
    warn = [[b.warning(w) for w in range(8)] for b in (lane, gen)]
    assert warn[0] == warn[1], f"warning counters differ: {warn[0]} vs {warn[1]}"
    assert warn[0][4] == 0 and warn[0][5] == 1 and warn[0][6] == 1
    twins = {e: oracle_env(po, model, qpos[e], qvel[e], ctrl[e], act[e], 3) for e in (5, 20, 0, 21, 69)}
    assert twins[5].warning(5) == 1 and twins[20].warning(6) == 1 and twins[0].warning(5) + twins[0].warning(6) == 0
    got = snapshot(lane)
    for e in (5, 20):
        assert np.all(got["act"][e] == 0), f"env {e}: mj_resetData zeroes act, got {got['act'][e]}"
        assert np.all(np.asarray(twins[e].act) == 0) and np.all(gen.get("act")[e] == 0)
        assert np.all(got["ctrl"][e] == 0)
    assert np.all(np.isfinite(got["qpos"])) and np.all(np.isfinite(got["qvel"]))
    against_generic(got, snapshot(gen), 1e-9, "after the resets")
    for e, d in twins.items():
        for f in FIELDS:
            _close(got[f][e], d.field(f), 1e-9, f"env {e} {f} against the oracle")
    others = np.ones(NENV, dtype=bool)
    others[[5, 20]] = False
    ref = snapshot(tidy)
    for f in EVERY:
        assert np.array_equal(got[f][others], ref[f][others]), f"a reset in the wavefront changed {f} of another lane"
    # later steps: ctrl written again (mj_resetData zeroed it), on this kernel and on the generic one, against the oracle continued
    ctrl2 = np.random.default_rng(17).uniform(-2.5, 2.5, ctrl.shape)
    for b, is_lane in ((lane, True), (gen, False)):
        b.set("ctrl", ctrl2)
        b.step(4)
        ran(b, is_lane)
    for e, d in twins.items():
        d.ctrl[:] = ctrl2[e]
        d.step(4)
    for b, name in ((lane, "lane = env"), (gen, "generic")):
        later = snapshot(b, FIELDS)
        for e, d in twins.items():
            for f in FIELDS:
                _close(later[f][e], d.field(f), 1e-9, f"four more steps on the {name} kernel, env {e} {f}")
    assert np.all(lane.get("act")[[5, 20]] != 0)
    for b in (lane, gen, tidy):
        b.close()


# ----------------------------------------------------------------------------------------------------------------------------- 7. flags
def test_disable_flags(oracle_built):
    from mujoco_ros_pkgs_amd import engine
    # mjDSBL_ACTUATION: act keeps its value bit for bit over 5 steps with non-zero ctrl (it lies inside the actranges), the forces are zero
    model = MODELS["A"](energy=True)
    model["disableflags"] = int(model["disableflags"]) | DSBL_ACTUATION
    cm = engine.CompiledModel(model)
    S = states("A", model)
    assert np.all(S[2] != 0)
    b = make(engine, cm, S)
    b.step(5)
    ran(b, True)
    got = snapshot(b)
    b.close()
    assert np.array_equal(got["act"], S[3])
    assert np.all(got["sensordata"][:, :2] == 0)  # (the two actuatorfrc sensors)
    against_oracle(oracle_built, model, got, S, 5, 1e-9, CHECK, "mjDSBL_ACTUATION")
    # mjDSBL_CLAMPCTRL: act_dot takes the raw ctrl
    for which in ("A", "B"):
        model = MODELS[which](energy=True)
        plain = engine.CompiledModel(model)
        model = MODELS[which](energy=True)
        model["disableflags"] = int(model["disableflags"]) | DSBL_CLAMPCTRL
        cm = engine.CompiledModel(model)
        S = states(which, model)
        res = []
        for c in (cm, plain):
            b = make(engine, c, S)
            b.step(1)
            ran(b, True)
            res.append(snapshot(b))
            b.close()
        against_oracle(oracle_built, model, res[0], S, 1, 1e-11, range(NENV), f"model {which}, mjDSBL_CLAMPCTRL")
        assert _err(res[0]["act"], res[1]["act"]) > 1e-4  # (the clamp does matter for these ctrl)


# ----------------------------------------------------------------------------------------------------------------------- 8. composition
@pytest.mark.parametrize("which", ["A", "B"])
def test_with_per_env_parameters(oracle_built, which):
    """Mode 2: per-env actuator gain / bias multiply act as they multiply ctrl; joint parameters per env too.  The four envs against their twins."""
    from mujoco_ros_pkgs_amd import engine
    base = MODELS[which](energy=True)
    cm = engine.CompiledModel(base)
    S = states(which, base)
    R = draw(base, NENV, 7, which=("joint", "actuator"))
    twins = {e: twin_model(base, R, e) for e in CHECK}
    for K, tol in ((1, 1e-11), (20, 1e-9)):
        b = make(engine, cm, S, mode=2)
        apply(b, R)
        b.step(K)
        ran(b, True)
        got = snapshot(b)
        b.close()
        against_oracle(oracle_built, base, got, S, K, tol, CHECK, f"model {which}, mode 2", models=twins)
    plain = make(engine, cm, S, mode=2)  # (the overlay matters: the same batch without it ends elsewhere)
    plain.step(20)
    assert _err(plain.get("qvel")[1:], got["qvel"][1:]) > 1e-6
    plain.close()


@pytest.mark.parametrize("which", ["A", "B"])
def test_with_wrenches(oracle_built, which):
    """The xfrc build: a wrench on every body, against the oracle and the generic kernel."""
    from mujoco_ros_pkgs_amd import engine
    model = MODELS[which](energy=True)
    cm = engine.CompiledModel(model)
    S = states(which, model)
    nb = int(model["nbody"])
    rng = np.random.default_rng(6)
    for K, tol, fs, ts in ((1, 1e-11, 30, 5), (20, 1e-9, 5, 1)):
        X = np.concatenate([rng.uniform(-fs, fs, (NENV, nb, 3)), rng.uniform(-ts, ts, (NENV, nb, 3))], axis=2).reshape(NENV, 6 * nb)
        res = []
        for mode in (1, 0):
            b = make(engine, cm, S, mode=mode)
            b.set_lane_env_xfrc(True)
            b.set("xfrc_applied", X)
            b.step(K)
            ran(b, mode == 1)
            res.append(snapshot(b))
            b.close()
        against_oracle(oracle_built, model, res[0], S, K, tol, range(NENV) if K == 1 else CHECK, f"model {which} with wrenches", xfrc=X)
        against_generic(res[0], res[1], 1e-9, f"model {which} with wrenches, {K} steps")
    free = make(engine, cm, S)
    free.step(20)
    assert _err(free.get("qvel"), res[0]["qvel"]) > 1e-6  # (the wrench does act)
    free.close()


# ------------------------------------------------------------------------------------------------------------------- 9. unchanged ground
def test_model_without_activations_still_runs(oracle_built):
    """franka_like (NA = 0: the compiled-in kernel), 70 envs, 20 steps in mode 1 against mode 0."""
    from conftest import random_franka_state
    from mujoco_ros_pkgs_amd import engine
    model = mjcf.load_asset("franka_like")
    cm = engine.CompiledModel(model)
    qpos, qvel = random_franka_state(model, NENV, 3)
    ctrl = np.random.default_rng(4).uniform(-3, 3, (NENV, model["nu"]))
    res = []
    for mode in (1, 0):
        b = engine.Batch(cm, NENV)
        b.set_lane_env(mode)
        b.set("qpos", qpos)
        b.set("qvel", qvel)
        b.set("ctrl", ctrl)
        b.step(20)
        assert bool(b.lane_env_info()[1]) == (mode == 1)
        res.append({f: b.get(f) for f in ("qpos", "qvel", "qacc", "sensordata")})
        b.close()
    for f in res[0]:
        _close(res[0][f], res[1][f], 1e-9, f"franka_like {f}, lane = env against the generic kernel")
