"""What solve_ik costs next to the route that existed before it ("Inverse kinematics"), at 4096 worlds, 16 updates per call (max_iters = 16, tol = 0, so every
world runs all of them), position and orientation of one site: the 5-joint arm of tests/ik_cases.py, and the packaged Fetch model with `dofs` set to its seven arm joints (if
BatchedSim takes it: a refusal is recorded with its message).  The other route is 16 x (forward() + site_jacp / site_jacr + torch.linalg.solve + the update of qpos in torch)
on the same stream.  The targets are the site poses of forward() at a nearby configuration.  Both routes in one process, alternating; a window is `reps` calls between two
device events, with `reps` chosen per route so that a window lasts at least --window seconds.  The figure is time per CALL (Python, argument checks, enqueue and kernels), not
kernel time.

    python tools/ik_probe.py --out profiles/ik_probe.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
FETCH_ARM = tuple("robot0:" + j for j in ("shoulder_pan_joint", "shoulder_lift_joint", "upperarm_roll_joint", "elbow_flex_joint", "forearm_roll_joint", "wrist_flex_joint", "wrist_roll_joint"))


def measure(a, model, site, dofs, spread):
    import torch

    import engine_matrix_cases as C
    import gymnasium_robotics_amd as grx

    N, kw = a.worlds, dict(damping=1e-2, max_step=0.5, tol=0.0, max_iters=a.iters, rot_weight=1.0, clamp_limits=True)
    sim = grx.BatchedSim(model, num_worlds=N, outputs=("site_xpos", "site_xmat", "site_jacp", "site_jacr"), jac_sites=(site,))
    sim.reset()
    dev, s, rng = sim.qpos.device, sim.site_id(site), np.random.default_rng(0)
    t = {k: np.asarray(model.tables[k]).reshape(-1) for k in ("jnt_type", "jnt_qposadr", "jnt_dofadr", "jnt_limited")}
    assert (t["jnt_type"] >= 2).all(), "the torch route below integrates hinge and slide joints only"
    move = np.zeros(sim.nv, bool)
    move[[sim.joint_dofadr(j) for j in dofs] if dofs else slice(None)] = True
    rnge = np.asarray(model.tables["jnt_range"], dtype=np.float64).reshape(-1, 2)
    lo, hi = (torch.tensor(np.where(t["jnt_limited"] != 0, rnge[:, k], (-1e30, 1e30)[k])[np.argsort(t["jnt_qposadr"])], dtype=torch.float32, device=dev) for k in (0, 1))
    sel = torch.tensor(move, dtype=torch.float32, device=dev)
    q0 = torch.minimum(torch.maximum(sim.qpos + sel * torch.tensor(rng.uniform(-spread, spread, (N, sim.nq)), dtype=torch.float32, device=dev), lo), hi)
    sim.qpos.copy_(torch.minimum(torch.maximum(q0 + sel * torch.tensor(rng.uniform(-spread, spread, (N, sim.nq)), dtype=torch.float32, device=dev), lo), hi))
    sim.forward()      # the targets: the site's pose at a configuration near the start
    tp, Rt = sim.site_xpos[:, s].clone().view(N, 1, 3), sim.site_xmat[:, s].clone().view(N, 3, 3)
    tq = torch.tensor(np.array([C.quat_from_mat(R) for R in Rt.cpu().numpy().astype(np.float64)]), dtype=torch.float32, device=dev).view(N, 1, 4)
    eye = kw["damping"] ** 2 * torch.eye(6, device=dev)

    def error():
        R = Rt @ sim.site_xmat[:, s].view(N, 3, 3).transpose(1, 2)
        v = 0.5 * torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
        sn, cs = v.norm(dim=-1, keepdim=True), 0.5 * (R.diagonal(dim1=1, dim2=2).sum(-1, keepdim=True) - 1)
        return torch.cat([tp[:, 0] - sim.site_xpos[:, s], torch.atan2(sn, cs) * v / sn.clamp_min(1e-20)], -1)

    def torch_route():      # every joint is a hinge or a slide: the update is an add and a clamp
        sim.qpos.copy_(q0)
        for _ in range(a.iters):
            sim.forward()
            J = torch.cat([sim.site_jacp[:, 0], sim.site_jacr[:, 0]], 1) * sel
            dq = (J.transpose(1, 2) @ torch.linalg.solve(J @ J.transpose(1, 2) + eye, error()[..., None])).squeeze(-1)
            dq = dq * (kw["max_step"] / dq.norm(dim=-1, keepdim=True).clamp_min(1e-20)).clamp_max(1.0)
            sim.qpos.copy_(torch.where(sel.bool(), torch.minimum(torch.maximum(sim.qpos + dq, lo), hi), sim.qpos))
        return sim.qpos

    out = (torch.empty_like(q0), torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev))
    routes = dict(solve_ik=lambda: sim.solve_ik(site, tp, tq, qpos0=q0, dofs=dofs, out=out, **kw)[0], forward_and_torch=torch_route)

    def window(f, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            f()
        t1.record()
        torch.cuda.synchronize()
        return 1e3 * t0.elapsed_time(t1) / reps      # microseconds per call

    got, reps = {}, {}
    for k, f in routes.items():      # warm-up, the route's answer, and the number of calls that fill a window
        window(f, 3)
        got[k] = f().clone()
        reps[k] = max(3, int(np.ceil(a.window * 1e6 / window(f, 5))))
    times = {k: [] for k in routes}
    for _ in range(a.rounds):      # alternating
        for k, f in routes.items():
            times[k].append(window(f, reps[k]))
    res = {k: dict(us=round(float(np.median(v)), 1), spread=round(float((max(v) - min(v)) / np.median(v)), 3), reps=reps[k]) for k, v in times.items()}
    res["solve_ik"]["median_err"] = float(out[1].median())
    torch_route()
    sim.forward()
    res["forward_and_torch"]["median_err"] = float(error().norm(dim=-1).median())
    res["max_abs_qpos_difference"] = float((got["solve_ik"] - got["forward_and_torch"]).abs().max())
    res["torch_over_solve_ik"] = round(res["forward_and_torch"]["us"] / res["solve_ik"]["us"], 1)
    sim.close()
    return res


def main():
    import torch

    import ik_cases as I
    from gymnasium_robotics_amd import _native
    from gymnasium_robotics_amd.envs.fetch import load_fetch_model

    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.25, help="least seconds of work between two device events")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    doc = dict(device=torch.cuda.get_device_name(0), build_id=_native.build_id(), worlds=a.worlds, updates=a.iters, window_s=a.window, rounds=a.rounds,
               unit="microseconds per CALL of 16 updates (Python, checks, enqueue and kernels; not kernel time): the median over the rounds of (device-event time of `reps` calls) / reps; "
                    "spread: (max - min) / median over the rounds")
    doc["arm"] = measure(a, I.model("arm"), "tip", None, 0.15)
    try:
        doc["fetch_arm"] = measure(a, load_fetch_model("FetchReach"), "robot0:grip", FETCH_ARM, 0.1)
    except (ValueError, RuntimeError, KeyError) as e:      # BatchedSim does not take the packaged model: say why
        doc["fetch_arm"] = dict(refused=f"{type(e).__name__}: {e}")
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
