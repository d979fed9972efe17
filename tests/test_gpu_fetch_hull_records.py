"""The hull-pair records (GrxModel::reci_hpair / recf_hpair: one record per candidate pair instead of the table walk of grx_mesh_pairs' set-up) and the site frames built only in
the pass the Fetch outputs read (GrxCtx::sites) change where values are loaded from and which passes compute values nobody reads -- never a result.  Every comparison here is
bit for bit, against the same library with the switch that restores the old path (GRX_NO_HULLPAIR_RECORDS at model creation, GRX_FETCH_SITES_EVERY_SUBSTEP at environment
creation)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
IDS = {"FetchPush": "FetchPush-v4", "FetchPickAndPlace": "FetchPickAndPlace-v4"}


def _env(task, n, **kw):
    import torch

    from gymnasium_robotics_amd.envs.fetch import FetchVecEnv

    assert torch.cuda.is_available(), "these tests need the GPU"
    return FetchVecEnv(IDS[task], num_envs=n, device="cuda:0", **kw)


def test_hull_pair_records_do_not_change_the_rollout(monkeypatch):
    """Free-running from the 168 folded-arm poses of the hull fixture (arm on head, wrist on the table: queued hull pairs, cached directions and portal searches in most substeps),
    30 steps of test_hull_candidate_lists_do_not_change_the_rollout's action schedule: models created with and without the records, each with and without the per-world hull rows,
    give bit-identical state rows and observations after every step."""
    import torch

    g = np.load(os.path.join(GOLDEN, "fetch_hull_teacher.npz"))
    n = g["obs"].shape[0]
    envs = []
    for rec_off, cache_off in ((False, False), (True, False), (False, True), (True, True)):
        for var, off in (("GRX_NO_HULLPAIR_RECORDS", rec_off), ("GRX_NO_HULLCACHE", cache_off)):
            if off:
                monkeypatch.setenv(var, "1")
            else:
                monkeypatch.delenv(var, raising=False)
        e = _env("FetchPickAndPlace", n, autoreset_mode="disabled", max_episode_steps=None, output="torch")
        assert (e.hullcache is None) == cache_off
        e.reset(seed=0)
        e.load_world_rows({k: g[k] for k in ("qpos", "qvel", "qacc_ws", "mocap", "aux", "goal")})
        envs.append(e)
    assert len({e._h.value for e in envs[:2]}) == 2      # two native models: one with the records, one without
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(3)
    a0 = torch.from_numpy(g["action"].astype(np.float32)).cuda()
    for t in range(30):
        a = a0 if t < 10 else (a0 * 0.2 + 0.3 * (torch.rand(n, 4, device="cuda:0", generator=gen) * 2 - 1))
        for e in envs:
            e.step(a)
        for k, e in enumerate(envs[1:]):
            assert torch.equal(envs[0].qpos, e.qpos) and torch.equal(envs[0].qvel, e.qvel) and torch.equal(envs[0].obs, e.obs), (t, k + 1)
    for e in (envs[0], envs[1]):
        used = e.hullcache[:, 21:].abs().sum(dim=1) > 0
        assert int(used.sum()) >= 20      # the path was really exercised: worlds with a persistent hull contact wrote their hint rows


@pytest.mark.parametrize("task", ["FetchPickAndPlace", "FetchPush"])
@pytest.mark.parametrize("parts", [1, 4])
def test_site_frames_only_where_they_are_read(monkeypatch, task, parts):
    """64 worlds, 12 steps of seeded random actions, unsplit and split in 4 parts (FetchPush: 21 passes, the last one the block_gripper callback's forward pass), episodes of 5 steps
    with staggered starts so that same-step autoresets (the reset kernel's forward pass, the terminal rows) fall inside: site frames in every pass against site frames in the last
    pass only -- every output row, state row, reward, flag, status word and terminal row is bit-identical after every step."""
    import torch

    n = 64
    monkeypatch.setenv("GRX_FETCH_SPLIT", str(parts))
    envs = []
    for every in (True, False):
        if every:
            monkeypatch.setenv("GRX_FETCH_SITES_EVERY_SUBSTEP", "1")
        else:
            monkeypatch.delenv("GRX_FETCH_SITES_EVERY_SUBSTEP", raising=False)
        e = _env(task, n, autoreset_mode="same_step", max_episode_steps=5, output="torch")
        assert e._split == parts and int(e._bufs.sites_every_substep) == int(every)
        e.reset(seed=11)
        e._elapsed[:] = np.arange(n) % 5
        envs.append(e)
    ref, lazy = envs
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(5)
    resets = 0
    for t in range(12):
        a = torch.rand(n, 4, device="cuda:0", generator=gen) * 2 - 1
        outs = [e.step(a) for e in envs]
        for name in ("obs", "achieved", "packed", "final_packed", "qpos", "qvel", "reward", "success", "status"):
            assert torch.equal(getattr(lazy, name), getattr(ref, name)), (t, name, int((getattr(lazy, name) != getattr(ref, name)).sum()))
        assert torch.equal(torch.as_tensor(outs[0][1]), torch.as_tensor(outs[1][1])) and torch.equal(torch.as_tensor(outs[0][3]), torch.as_tensor(outs[1][3])), t
        resets += int(torch.as_tensor(outs[0][3]).sum())
    assert resets >= n      # same-step autoresets happened: final_packed held terminal rows when it was compared
    assert float(ref.final_packed.abs().sum()) > 0
