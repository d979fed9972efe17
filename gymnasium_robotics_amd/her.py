"""Hindsight-experience-replay storage and relabelling on the device -- the caller of ``GoalEnv.compute_reward``.

The reference documents the use (README.md:72-76, gymnasium_robotics/core.py:45-67): "substitute a goal and recompute the reward":

    env.unwrapped.compute_reward(obs["achieved_goal"], substituted_goal, info)

With thousands of worlds stepped per launch, doing that through the host would move every trajectory over PCIe.  Here the episode rows the step
kernels already write (``env.packed`` = ``[obs | achieved | desired | reward | success]`` per world) are appended to a device buffer, and ONE kernel
(``grx_her_relabel``) gathers a batch of transitions, substitutes the goals ("future" strategy: a goal achieved later in the same episode, with
probability k / (k + 1)), recomputes reward and success with the device functions behind ``compute_reward`` and writes packed replay rows

    [obs_t | achieved_t | goal | action_t | reward | obs_t+1 | achieved_t+1 | success]

into a device ring buffer.  Nothing leaves HBM; the learner reads ``replay.rows``.
"""
import ctypes
import os
from typing import Optional

import numpy as np
import torch

from . import _native

FETCH, HAND_REACH, MAZE, MANIPULATE = 0, 1, 2, 3


def reward_spec(env) -> dict:
    """kind / thresholds / flags of grx_her_relabel for a goal-conditioned device environment (the same parameters its compute_reward uses)"""
    name = type(env).__name__
    sparse = int(getattr(env, "reward_type", "sparse") == "sparse")
    if name == "FetchVecEnv":
        return dict(kind=FETCH, p0=float(env.task.distance_threshold), p1=0.0, sparse=sparse)
    if name == "HandReachVecEnv":
        return dict(kind=HAND_REACH, p0=float(env.distance_threshold), p1=0.0, sparse=sparse)
    if name in ("PointMazeVecEnv", "AntMazeVecEnv"):
        return dict(kind=MAZE, p0=0.45, p1=0.0, sparse=sparse)
    if name == "HandBlockVecEnv":   # the arguments of its grx_manip_compute_reward call (envs/hand.py:_launch_reward)
        from .envs.manipulate_spec import ROTATION_THRESHOLD

        return dict(kind=MANIPULATE, p0=float(env.distance_threshold), p1=float(ROTATION_THRESHOLD), sparse=sparse, ignore_pos=int(env.target_position == "ignore"),
                    ignore_rot=int(env.target_rotation == "ignore"), ignore_z=int(env._objcfg["ignore_z_target_rotation"]))
    raise TypeError(f"{name} is not a goal-conditioned environment")


class HerReplay:
    """A ring of the last `horizon` + 1 output rows of every world + the actions that led to them + a replay ring [capacity, OW], all on the
    environment's device.  Episodes may start at different steps in different worlds (same-step autoreset): `episode_start[w]` is the row at which
    world w's current episode began, and only rows of the current episode that are still in the ring are sampled.

        buf = HerReplay(env, horizon=50, capacity=1 << 20)
        obs, _ = env.reset(seed=0); buf.begin_episode(env.packed)
        for t in range(50):
            obs, r, term, trunc, info = env.step(a); buf.append(a, env.packed)        # append(..., reset_mask) when worlds were autoreset in this step
        buf.relabel(batch=4 * env.num_envs, k_future=4)        # one kernel: gather + goal substitution + reward recompute + replay write
    """

    def __init__(self, env, horizon: int, capacity: int, obs_dim: Optional[int] = None, goal_dim: Optional[int] = None, seed: int = 0, continuous: bool = False):
        self.env, self.T, self.N = env, int(horizon), int(env.num_envs)
        self.device = env.device
        self.W = int(env.packed.shape[1])
        self.goal_dim = int(goal_dim if goal_dim is not None else env.single_observation_space["desired_goal"].shape[0])
        self.obs_dim = int(obs_dim if obs_dim is not None else self.W - 2 * self.goal_dim - 2)
        self.act_dim = int(env.single_action_space.shape[0])
        self.OW = 2 * self.obs_dim + 3 * self.goal_dim + self.act_dim + 2
        self.spec = reward_spec(env)
        self.continuous = bool(continuous)        # False: append() past `horizon` steps is an error (one episode per buffer); True: the ring wraps
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=self.device)
        self.R = self.T + 1
        self.episode, self.actions = z(self.R, self.N, self.W), z(self.R, self.N, self.act_dim)   # actions[r] = the action that led to row r
        self.episode_start = z(self.N, dtype=torch.int32)
        # same-step autoreset with final_rows (append): where world w's previous episode began, and the absolute row index its terminal row belongs to (-1: none)
        self.prev_start, self.term_t = z(self.N, dtype=torch.int32), torch.full((self.N,), -1, dtype=torch.int32, device=self.device)
        self._final_rows = None                    # the env's [N, W] buffer of terminal rows (e.g. FetchVecEnv.final_packed); read by the relabel kernel, never copied
        self._just_ended = np.zeros(self.N, bool)  # host mirror of term_t == t
        self._start_host = np.zeros(self.N, np.int64)          # host mirror of episode_start: decides without a device sync whether anything can be sampled
        self.rows, self.capacity, self.head, self.size = z(int(capacity), self.OW), int(capacity), 0, 0
        self.t = 0                                 # absolute index of the newest row
        self._seed, self._calls = int(seed), 0     # counter-based index stream (grx_her_sample): see reseed()
        self._L = _native.lib()
        # one kernel per append (grx_her_append) and one per relabel (grx_her_draw_relabel); GRX_FETCH_FUSED_TAIL=0: the copies, the mark kernel and the sample + relabel pair
        self._fused = os.environ.get("GRX_FETCH_FUSED_TAIL", "1") != "0"
        self._last_list = None
        # reset masks reach the device through pinned buffers: a copy from pageable memory would make the host wait for the step kernel (core.PinnedStager)
        self._mask_pin = [dict(buf=torch.empty(self.N, dtype=torch.bool, pin_memory=True), event=None) for _ in range(4)]
        self._mask_next, self._mask_dev = 0, torch.zeros(self.N, dtype=torch.bool, device=self.device)

    # ---------------------------------------------------------------- episode storage (device copies of what the step kernel wrote)
    def begin_episode(self, packed_rows: torch.Tensor):
        self.episode[0].copy_(packed_rows)
        self.episode_start.zero_()
        self.prev_start.zero_(); self.term_t.fill_(-1)
        self._start_host[:] = 0
        self._just_ended[:] = False
        self.t = 0

    def append(self, actions: torch.Tensor, packed_rows: torch.Tensor, reset_mask: Optional[torch.Tensor] = None, final_rows: Optional[torch.Tensor] = None):
        """row t + 1 <- the rows of this step.  reset_mask (bool [N]): worlds that were autoreset inside this step -- their row is the first one of a new
        episode.  final_rows ([N, W] device buffer whose row w holds the TERMINAL packed row of a world reset in this step, e.g. FetchVecEnv.final_packed):
        the finished episode stays sampleable for this one step WITH its last transition (next observation = the terminal row), which is how a replay that
        stores whole episodes sees it (/root/reference/README.md:66-76).  Without final_rows that last transition is not stored."""
        if self.t >= self.T and not self.continuous:
            raise RuntimeError("episode buffer is full: call begin_episode()")
        self.t += 1
        r = self.t % self.R
        if self._fused:
            return self._append_fused(r, actions, packed_rows, reset_mask, final_rows)
        self.actions[r].copy_(actions)
        self.episode[r].copy_(packed_rows)
        if reset_mask is not None:     # bool [N]: numpy / CPU tensor (what the envs return) or a device tensor
            host = reset_mask.cpu().numpy() if isinstance(reset_mask, torch.Tensor) else np.asarray(reset_mask)
            self._start_host[host.astype(bool)] = self.t
            if isinstance(reset_mask, torch.Tensor) and reset_mask.device == self.device:
                dev = reset_mask
            else:
                slot = self._mask_pin[self._mask_next]
                self._mask_next = (self._mask_next + 1) % len(self._mask_pin)
                if slot["event"] is not None:
                    slot["event"].synchronize()
                slot["buf"].numpy()[:] = host.astype(bool)
                dev = self._mask_dev
                dev.copy_(slot["buf"], non_blocking=True)
                slot["event"] = torch.cuda.Event()
                slot["event"].record(torch.cuda.current_stream(self.device))
            if final_rows is not None:
                assert tuple(final_rows.shape) == (self.N, self.W) and final_rows.is_contiguous()
                self._final_rows = final_rows
            track = self._final_rows is not None
            self._just_ended = host.astype(bool) if track else self._just_ended
            _native.check(self._L.grx_her_mark_resets(dev.data_ptr(), self.N, self.t, self.episode_start.data_ptr(), self.prev_start.data_ptr() if track else None,
                                                      self.term_t.data_ptr() if track else None, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        elif self._final_rows is not None:
            self._just_ended = np.zeros(self.N, bool)

    def _upload_mask(self, host):
        slot = self._mask_pin[self._mask_next]
        self._mask_next = (self._mask_next + 1) % len(self._mask_pin)
        if slot["event"] is not None:
            slot["event"].synchronize()
        slot["buf"].numpy()[:] = host
        self._mask_dev.copy_(slot["buf"], non_blocking=True)
        slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream(self.device))
        return self._mask_dev

    def _append_fused(self, r, actions, packed_rows, reset_mask, final_rows):
        """append() as ONE kernel (grx_her_append): both row copies and the episode marks of the reset worlds.  Those are read from the index list the environment left on the
        device (`env.step_reset_list`: int32 tensor + host count, e.g. FetchVecEnv) when its count agrees with reset_mask; otherwise from the mask (uploaded if it is a host array)."""
        dev_rows = lambda x, shape: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(device=self.device, dtype=torch.float32).contiguous().view(shape)
        acts, rows = dev_rows(actions, (self.N, self.act_dim)), dev_rows(packed_rows, (self.N, self.W))
        a = _native.HerAppendArgsStruct()
        a.packed, a.action, a.row_dst, a.act_dst = rows.data_ptr(), acts.data_ptr(), self.episode[r].data_ptr(), self.actions[r].data_ptr()
        a.n_row, a.n_act, a.n_worlds, a.t, a.W = self.N * self.W, self.N * self.act_dim, self.N, self.t, self.W
        a.start = self.episode_start.data_ptr()
        keep = None      # (a device mask made here stays alive until the launch is enqueued)
        if reset_mask is not None:
            host = (reset_mask.cpu().numpy() if isinstance(reset_mask, torch.Tensor) else np.asarray(reset_mask)).astype(bool)
            self._start_host[host] = self.t
            if final_rows is not None:
                assert tuple(final_rows.shape) == (self.N, self.W) and final_rows.is_contiguous()
                self._final_rows = final_rows
            track = self._final_rows is not None
            self._just_ended = host if track else self._just_ended
            if track:
                a.prev_start, a.term_t = self.prev_start.data_ptr(), self.term_t.data_ptr()
            count, lst = int(host.sum()), getattr(self.env, "step_reset_list", None)
            if lst is self._last_list:      # the environment publishes a fresh tuple with every step: the one an earlier append consumed is stale
                lst = None
            self._last_list = lst
            if count == 0:
                pass
            elif lst is not None and lst[1] == count and lst[0].dtype == torch.int32 and lst[0].device == self.device:
                a.list, a.count = lst[0].data_ptr(), count
            elif isinstance(reset_mask, torch.Tensor) and reset_mask.device == self.device:
                keep = reset_mask if reset_mask.dtype in (torch.bool, torch.uint8) else reset_mask.bool()
                a.mask = keep.data_ptr()
            else:
                a.mask = self._upload_mask(host).data_ptr()
        elif self._final_rows is not None:
            self._just_ended = np.zeros(self.N, bool)
        _native.check(self._L.grx_her_append(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def set_episode_start(self, starts):
        """absolute row at which every world's current episode began (e.g. negative values for episodes that were already under way at row 0)"""
        self._start_host[:] = np.asarray(starts, dtype=np.int64)
        self.episode_start.copy_(torch.from_numpy(self._start_host.astype(np.int32)).to(self.device))

    # ---------------------------------------------------------------- sampling + the fused relabel kernel
    def reseed(self, seed: int):
        """restart the index stream: the same (seed, number of sample_indices calls since) reproduces the same draws"""
        self._seed, self._calls = int(seed), 0

    def _can_sample(self) -> bool:
        """host mirror: does any world have a transition in the ring (of its current episode, or of the one that ended in this step when terminal rows are kept)"""
        track = self._final_rows is not None
        return bool(((np.maximum(self._start_host, max(self.t - self.T, 0)) < self.t) | (self._just_ended if track else False)).any())

    def sample_indices(self, batch: int, k_future: int = 4):
        """(t, world, t_goal): a uniform world, a uniform transition of that world's current episode among the rows still in the ring; with
        probability k / (k + 1) the goal achieved at a uniformly drawn LATER row of the same episode (the "future" strategy of Andrychowicz et al.
        2017), else -1 = keep the episode's goal.  Worlds whose episode has no transition yet (just reset) are not drawn.  One kernel
        (grx_her_sample) with a counter-based generator; None when nothing can be sampled."""
        track = self._final_rows is not None
        if not self._can_sample():
            return None                                                                   # every world has just been reset: nothing to sample
        t, w, tg = (torch.empty(batch, dtype=torch.int32, device=self.device) for _ in range(3))
        _native.check(self._L.grx_her_sample_final(self.episode_start.data_ptr(), self.prev_start.data_ptr() if track else None, self.term_t.data_ptr() if track else None,
                                                   self.N, self.t, self.T, int(k_future), self._seed, self._calls, batch,
                                                   t.data_ptr(), w.data_ptr(), tg.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._calls += 1
        return t, w, tg

    def _her_args(self, out: torch.Tensor):
        a = _native.HerArgsStruct()
        a.rows, a.acts, a.out = self.episode.data_ptr(), self.actions.data_ptr(), out.data_ptr()
        a.T, a.N, a.W, a.obs_dim, a.goal_dim, a.act_dim = self.T, self.N, self.W, self.obs_dim, self.goal_dim, self.act_dim   # ring of T + 1 rows
        if self._final_rows is not None:
            a.term_rows, a.term_t = self._final_rows.data_ptr(), self.term_t.data_ptr()
        for k, v in self.spec.items():
            setattr(a, k, v)
        return a

    def relabel_into(self, out: torch.Tensor, t: torch.Tensor, w: torch.Tensor, t_goal: torch.Tensor):
        """the kernel alone: out[b] <- relabelled transition (t[b], w[b], t_goal[b]); int32 index tensors on the device"""
        a = self._her_args(out)
        a.t_idx, a.w_idx, a.t_goal = t.data_ptr(), w.data_ptr(), t_goal.data_ptr()
        assert out.is_contiguous() and tuple(out.shape) == (len(t), self.OW) and t.dtype == w.dtype == t_goal.dtype == torch.int32
        _native.check(self._L.grx_her_relabel(ctypes.byref(a), len(t), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    def relabel(self, batch: int, k_future: int = 4):
        """sample + relabel + write `batch` rows at the head of the replay ring; returns the view of the rows just written"""
        if batch > self.capacity:
            raise ValueError("batch larger than the replay capacity")
        if self.head + batch > self.capacity:
            self.head = 0                                    # keep every batch contiguous (a ring of whole batches)
        view = self.rows[self.head: self.head + batch]
        if self._fused:      # the draws of sample_indices and the rows of relabel_into in one kernel: no index tensors
            if not self._can_sample():
                return self.rows[self.head: self.head]
            track = self._final_rows is not None
            _native.check(self._L.grx_her_draw_relabel(ctypes.byref(self._her_args(view)), self.episode_start.data_ptr(), self.prev_start.data_ptr() if track else None,
                                                       self.t, int(k_future), self._seed, self._calls, batch, None,
                                                       ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
            self._calls += 1
        else:
            idx = self.sample_indices(batch, k_future)
            if idx is None:
                return self.rows[self.head: self.head]
            self.relabel_into(view, *idx)
        self.head += batch
        self.size = min(self.capacity, max(self.size, self.head))
        return view

    # ---------------------------------------------------------------- views of a replay row
    def split(self, rows: torch.Tensor) -> dict:
        o, g, a = self.obs_dim, self.goal_dim, self.act_dim
        c = np.cumsum([0, o, g, g, a, 1, o, g, 1])
        names = ("observation", "achieved_goal", "desired_goal", "action", "reward", "next_observation", "next_achieved_goal", "success")
        return {n: rows[:, c[i]: c[i + 1]] for i, n in enumerate(names)}


class EpisodicHerReplay(HerReplay):
    """HerReplay + a device store of FINISHED episodes (grx_her_archive, grx_her_episode_sample: include/grx_capi.h).  The ring of HerReplay only holds episodes that are
    still running; here every episode that ends moves, rows and actions, into one of `episodes` slots [episodes, horizon + 1, W] before the step that ended it is appended,
    and `sample` draws relabelled transitions from whole episodes -- "future" goals from the whole rest of the episode, "final" and "episode" goals, a fresh relabel of old
    experience at every call -- in the row format `relabel` writes.  HerReplay's own ring, marks and draws are untouched by the store.

        buf = EpisodicHerReplay(env, horizon=50, capacity=1 << 20, episodes=1 << 16, continuous=True)
        ... buf.append(a, env.packed, done, final_rows=env.final_packed)      # archives the worlds of `done`, then HerReplay.append
        rows = buf.sample(4 * env.num_envs, k_future=4, strategy="future")
    """
    STRATEGIES = {"future": 0, "final": 1, "episode": 2}

    def __init__(self, env, horizon: int, capacity: int, episodes: int, **kw):
        if int(episodes) < int(env.num_envs):
            raise ValueError(f"episodes = {episodes} is less than the number of worlds {env.num_envs}: one step can end an episode in every world")
        if int(episodes) >= 1 << 31:
            raise ValueError("episodes must be below 2^31")
        super().__init__(env, horizon, capacity, **kw)
        self.E = int(episodes)
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=self.device)
        self.ep_rows, self.ep_acts = z(self.E, self.R, self.W), z(self.E, self.R, self.act_dim)      # ep_acts[e, j] = the action that led to row j of episode e
        self.ep_meta, self.ep_count = z(self.E, 4, dtype=torch.int32), z(1, dtype=torch.int64)         # {len, world, first_row, 0}; episodes archived so far (device)
        self.archived = 0                          # host mirror of ep_count: decides without a device sync whether anything can be sampled
        self._sample_seed, self._sample_calls = self._seed, 0
        self._sample_valid = z(1, dtype=torch.int32)
        self._list_pin = [dict(buf=torch.empty(self.N, dtype=torch.int32, pin_memory=True), event=None) for _ in range(4)]
        self._list_next, self._list_dev = 0, z(self.N, dtype=torch.int32)

    def _upload_list(self, worlds):
        slot = self._list_pin[self._list_next]
        self._list_next = (self._list_next + 1) % len(self._list_pin)
        if slot["event"] is not None:
            slot["event"].synchronize()
        slot["buf"].numpy()[:len(worlds)] = worlds
        self._list_dev[:len(worlds)].copy_(slot["buf"][:len(worlds)], non_blocking=True)
        slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream(self.device))
        return self._list_dev

    def append(self, actions: torch.Tensor, packed_rows: torch.Tensor, reset_mask: Optional[torch.Tensor] = None, final_rows: Optional[torch.Tensor] = None):
        """HerReplay.append, after the episodes of the worlds in reset_mask have been moved into the store (one grx_her_archive launch pair, issued BEFORE the append: it
        reads the ring before this step's row overwrites the oldest one, and the episode marks before these worlds are re-marked).  With terminal rows (final_rows, now or in
        an earlier call) the stored episode ends with the terminal row and this step's action; without, with the newest ring row."""
        if self.t >= self.T and not self.continuous:
            raise RuntimeError("episode buffer is full: call begin_episode()")
        if reset_mask is not None:
            host = (reset_mask.cpu().numpy() if isinstance(reset_mask, torch.Tensor) else np.asarray(reset_mask)).astype(bool)
            count = int(host.sum())
            if count:
                actions = (actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions))).to(device=self.device, dtype=torch.float32).contiguous().view(self.N, self.act_dim)
                term = final_rows if final_rows is not None else self._final_rows
                a = _native.HerArchiveArgsStruct()
                a.rows, a.acts, a.start = self.episode.data_ptr(), self.actions.data_ptr(), self.episode_start.data_ptr()
                a.n_worlds, a.T, a.W, a.act_dim, a.t_prev, a.count = self.N, self.T, self.W, self.act_dim, self.t, count
                lst = getattr(self.env, "step_reset_list", None)
                if lst is self._last_list:      # (HerReplay._append_fused: the tuple an earlier append consumed is stale; super().append records this one)
                    lst = None
                if lst is not None and lst[1] == count and lst[0].dtype == torch.int32 and lst[0].device == self.device:
                    a.list = lst[0].data_ptr()
                else:
                    a.list = self._upload_list(np.nonzero(host)[0].astype(np.int32)).data_ptr()
                if term is not None:
                    assert tuple(term.shape) == (self.N, self.W) and term.is_contiguous()
                    a.final_rows, a.step_action, a.final_compact = term.data_ptr(), actions.data_ptr(), 0
                a.ep_rows, a.ep_acts, a.ep_meta, a.ep_count, a.episodes = self.ep_rows.data_ptr(), self.ep_acts.data_ptr(), self.ep_meta.data_ptr(), self.ep_count.data_ptr(), self.E
                _native.check(self._L.grx_her_archive(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
                self.archived += count
        return super().append(actions, packed_rows, reset_mask, final_rows)

    def reseed_samples(self, seed: int):
        """restart the index stream of sample(): the same (seed, number of sample calls since) reproduces the same draws; relabel's stream is not touched"""
        self._sample_seed, self._sample_calls = int(seed), 0

    def sample(self, batch: int, k_future: int = 4, strategy: str = "future", out: Optional[torch.Tensor] = None):
        """[batch, OW] relabelled transitions drawn from the stored episodes in one kernel: a uniform stored episode, a uniform transition t of it, and with probability
        k / (k + 1) a substituted goal -- "future": achieved at a uniform later row t + 1 .. L, "final": at the last row, "episode": at a uniform row 0 .. L.  Nothing
        archived yet: an empty view, and the stream does not advance (as relabel)."""
        if strategy not in self.STRATEGIES:
            raise ValueError(f"unknown strategy {strategy!r}: one of {sorted(self.STRATEGIES)}")
        if batch < 1 or k_future < 0:
            raise ValueError("batch >= 1 and k_future >= 0")
        if out is None:
            out = torch.empty(batch, self.OW, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and tuple(out.shape) == (batch, self.OW) and out.dtype == torch.float32
        if self.archived == 0:
            return out[:0]
        _native.check(self._L.grx_her_episode_sample(ctypes.byref(self._her_args(out)), self.ep_rows.data_ptr(), self.ep_acts.data_ptr(), self.ep_meta.data_ptr(),
                                                     self.ep_count.data_ptr(), self.E, self.STRATEGIES[strategy], int(k_future), self._sample_seed, self._sample_calls, batch,
                                                     out.data_ptr(), self._sample_valid.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        self._sample_calls += 1
        return out

    def store_views(self):
        """(rows [E, T+1, W], actions [E, T+1, act_dim], meta [E, 4] int32 = {len, world, first_row, 0}, count [1] int64): the device tensors of the store"""
        return self.ep_rows, self.ep_acts, self.ep_meta, self.ep_count


class Normalizer:
    """Running per-component mean and standard deviation of observations and goals, kept on the device from relabelled HER batches, and their application -- the
    normaliser of the DDPG + HER recipe (Andrychowicz et al. 2017; Plappert et al. 2018): (x - mean) / std clipped to +-clip.

        norm = Normalizer(buf)                       # a HerReplay / EpisodicHerReplay, or the environment itself
        rows = buf.relabel(batch=256)
        norm.update(rows)                            # obs_t and the relabelled goal of every row -> fp64 sums; mean / inv_std refreshed (two launches)
        x = norm.normalize(rows)                     # obs and goal columns normalised, action / reward / success copied (one launch; out=rows: in place)
        actor_in = norm.policy_input(env.packed)     # [N, obs_dim + goal_dim] = [norm(obs) | norm(desired)]

    A thin caller of the grx_normstat entry points of libgrx_hip.so (include/grx_capi.h), which define the arithmetic: sums in fp64 in a fixed order with no floating-point
    atomics (bit-identical from run to run), a row with a non-finite tracked value skipped and counted, a NaN input staying a NaN.  `valid` is the device word of a C-side
    batch (grx_replay_batch.valid): zero means "this slot holds nothing" and is read by the kernels."""

    def __init__(self, replay_or_env, eps: float = 1e-2, clip: float = 5.0):
        src = replay_or_env
        if isinstance(src, HerReplay):
            self.device, self.obs_dim, self.goal_dim, self.act_dim, self.W = src.device, src.obs_dim, src.goal_dim, src.act_dim, src.W
        else:
            self.device, self.W = src.device, int(src.packed.shape[1])
            self.goal_dim = int(src.single_observation_space["desired_goal"].shape[0])
            self.obs_dim = self.W - 2 * self.goal_dim - 2
            self.act_dim = int(src.single_action_space.shape[0])
        if not (eps > 0 and clip > 0):
            raise ValueError("eps and clip must be positive")
        self.eps, self.clip = float(eps), float(clip)
        self.D = self.obs_dim + self.goal_dim
        self.OW = 2 * self.obs_dim + 3 * self.goal_dim + self.act_dim + 2
        self._L = _native.lib()
        lay = (ctypes.c_int64 * 8)()
        _native.check(self._L.grx_normstat_layout(self.obs_dim, self.goal_dim, lay))
        self._block = torch.zeros(int(lay[7]), dtype=torch.uint8, device=self.device)      # the stat block: statistics, then the update's workspace
        view = lambda off, n, size, dtype: self._block[int(off): int(off) + n * size].view(dtype)
        self.sum, self.sumsq = view(lay[0], self.D, 8, torch.float64), view(lay[1], self.D, 8, torch.float64)
        self._count, self._skipped = view(lay[2], 1, 8, torch.int64), view(lay[3], 1, 8, torch.int64)
        self.mean, self.inv_std = view(lay[4], self.D, 4, torch.float32), view(lay[5], self.D, 4, torch.float32)
        self._refresh()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _refresh(self):
        _native.check(self._L.grx_normstat_refresh(self._block.data_ptr(), self.obs_dim, self.goal_dim, self.eps, self._stream()))

    def _check_rows(self, rows, width, what):
        if not (rows.dim() == 2 and rows.shape[1] == width and rows.dtype == torch.float32 and rows.is_contiguous() and rows.device == self._block.device):
            raise ValueError(f"{what}: a contiguous float32 [batch, {width}] tensor on {self._block.device} is expected")

    def update(self, rows: torch.Tensor, valid: Optional[torch.Tensor] = None):
        """add replay rows [batch, OW] to the statistics; valid: None or a device int32 [1] whose zero means "nothing in this slot" (decided by the kernels)"""
        self._check_rows(rows, self.OW, "update")
        if len(rows) == 0:      # the empty view of HerReplay.relabel when nothing can be sampled
            return
        if valid is not None and not (valid.dtype == torch.int32 and valid.numel() >= 1 and valid.device == self._block.device):
            raise ValueError("update: valid is a device int32 [1] tensor")
        _native.check(self._L.grx_normstat_update(self._block.data_ptr(), rows.data_ptr(), len(rows), self.OW, self.obs_dim, self.goal_dim,
                                                  valid.data_ptr() if valid is not None else None, self.eps, self._stream()))

    def normalize(self, rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """replay rows with the observation and goal columns normalised and clipped, the others copied; out=rows normalises in place"""
        self._check_rows(rows, self.OW, "normalize")
        if out is None:
            out = torch.empty_like(rows)
        self._check_rows(out, self.OW, "normalize(out=)")
        if out.shape != rows.shape:
            raise ValueError("normalize: out has another batch size")
        if len(rows):
            _native.check(self._L.grx_normstat_apply_batch(self._block.data_ptr(), rows.data_ptr(), len(rows), self.OW, self.obs_dim, self.goal_dim, self.act_dim, self.clip,
                                                           out.data_ptr(), self._stream()))
        return out

    def policy_input(self, packed: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n, obs_dim + goal_dim] = [norm(obs) | norm(desired)] of packed environment rows (env.packed)"""
        self._check_rows(packed, self.W, "policy_input")
        if out is None:
            out = torch.empty(len(packed), self.D, dtype=torch.float32, device=self.device)
        self._check_rows(out, self.D, "policy_input(out=)")
        if len(out) != len(packed):
            raise ValueError("policy_input: out has another number of rows")
        if len(packed):
            _native.check(self._L.grx_normstat_apply_packed(self._block.data_ptr(), packed.data_ptr(), len(packed), self.W, self.obs_dim, self.goal_dim, self.clip,
                                                            out.data_ptr(), self._stream()))
        return out

    @property
    def std(self) -> torch.Tensor:
        return 1.0 / self.inv_std

    @property
    def count(self) -> int:
        """rows counted so far (reads the device word: waits for the stream)"""
        return int(self._count.item())

    @property
    def skipped(self) -> int:
        """rows left out because a tracked value was not finite (reads the device word)"""
        return int(self._skipped.item())

    def state_dict(self) -> dict:
        """what a resumed run needs: the fields of the C ABI's state blob (env_capi.pack_norm_state)"""
        return dict(obs_dim=self.obs_dim, goal_dim=self.goal_dim, eps=self.eps, clip=self.clip, sum=self.sum.cpu(), sumsq=self.sumsq.cpu(), count=self.count, skipped=self.skipped)

    def load_state_dict(self, state: dict):
        if (int(state["obs_dim"]), int(state["goal_dim"])) != (self.obs_dim, self.goal_dim):
            raise ValueError(f"state of dimensions ({state['obs_dim']}, {state['goal_dim']}), normalizer of ({self.obs_dim}, {self.goal_dim})")
        if not (state["eps"] > 0 and state["clip"] > 0):
            raise ValueError("eps and clip must be positive")
        self.eps, self.clip = float(state["eps"]), float(state["clip"])
        self.sum.copy_(torch.as_tensor(state["sum"], dtype=torch.float64).reshape(self.D))
        self.sumsq.copy_(torch.as_tensor(state["sumsq"], dtype=torch.float64).reshape(self.D))
        self._count.fill_(int(state["count"]))
        self._skipped.fill_(int(state["skipped"]))
        self._refresh()      # mean / inv_std by the refresh code of update
