"""League training: every env of a self-play rollout races its own opponent.

``SelfPlayPPO`` (agent/self_play_ppo.py:40-50) draws ONE frozen snapshot per
update with np.random.choice and all envs race it for the whole rollout.  Here
the pool lives in a policy bank on the device, every env holds the id of its
own opponent, the outcome of every finished episode is counted where it happens
and the next opponent is drawn at once -- weighted towards the snapshots the
learner still loses to (prioritised fictitious self-play).  Nothing goes through
the host: ids, tallies and the sampling table are small device arrays and the
rollout stays one library call (rx_league_rollout_steps, include/rx.h).

``PoolSlots``          which bank slot holds which snapshot (host bookkeeping);
``LeagueVectorEnv``    SelfPlayVectorEnv with the bank, ``opp_id``, ``draw_count``,
                       ``tally``, ``cdf`` and the per-step path;
``LeagueStepRollout``  the rx_league_rollout_steps driver (graph-capturable);
``LeagueSelfPlayPPO``  the trainer: SelfPlayPPO's cadence, checkpoints and pool
                       list, with the bank kept beside it.

The rules (sampling table, draw, tally) are csrc/rx_league.h; DESIGN.md §4.
"""
import ctypes

import torch

from . import _lib
from . import dist as rdist
from .league import STRIDE_ALIGN
from .ppo import PPO
from .ppo_fused import SelfPlayStepRollout, policy_supported
from .selfplay import SelfPlayPPO, SelfPlayVectorEnv

MAX_SLOTS = _lib.RX_LEAGUE_MAX_SLOTS


class PoolSlots:
    """Snapshot number s (0, 1, 2, ... in the order taken) lives in bank slot
    s % pool_size, so a row of the bank never moves: the FIFO's oldest member is
    the one the next snapshot overwrites.  The live slots are always 0 ..
    n_live - 1."""

    def __init__(self, pool_size, n_snapshots=0):
        if not 1 <= int(pool_size) <= MAX_SLOTS:
            raise ValueError(f"pool_size={pool_size}: the league bank holds 1..{MAX_SLOTS} snapshots")
        self.pool_size = int(pool_size)
        self.n_snapshots = int(n_snapshots)

    def slot_of(self, s):
        return int(s) % self.pool_size

    @property
    def n_live(self):
        return min(self.n_snapshots, self.pool_size)

    def push(self):
        """Take the next snapshot number: (s, its slot, whether the slot held an older snapshot)."""
        s = self.n_snapshots
        self.n_snapshots += 1
        return s, self.slot_of(s), s >= self.pool_size

    def members(self):
        """Snapshot numbers in the pool, oldest first (the order of ``opponent_pool``)."""
        return list(range(max(0, self.n_snapshots - self.pool_size), self.n_snapshots))

    def member_slots(self):
        return [self.slot_of(s) for s in self.members()]


def flat_policy_copy(agent):
    """A COPY of the agent's parameters as one flat tensor (a bank row's source).  Not
    rx.evaluate._flat_policy, which returns the module's own storage when it is packed."""
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()])


class LeagueVectorEnv(SelfPlayVectorEnv):
    """N two-car envs, car ``agent_idx`` the learner's, the other car of env e
    driven by bank member ``opp_id[e]``.  While no slot is live the opponent is
    SelfPlayVectorEnv's random one.

    The per-step path (``step_device``): rx_policy_act_bank on the opponent rows
    with the current ids, the step with the info columns, then rx_league_draw of the
    step's done flags -- what rx_league_rollout_steps enqueues per step."""

    def __init__(self, venv, agent_idx=0, seed=0, pool_size=5, prec=_lib.RX_PREC_FP32):
        super().__init__(venv, agent_idx, seed)
        if venv.D != 19:
            raise ValueError(f"league training needs the 19-column two-car observation (got {venv.D})")
        if not 1 <= int(pool_size) <= MAX_SLOTS:
            raise ValueError(f"pool_size={pool_size}: the league bank holds 1..{MAX_SLOTS} snapshots")
        self.L = _lib.load()
        self.pool_size, self.prec, self.seed = int(pool_size), int(prec), int(seed) & (2**64 - 1)
        n, dev = self.num_envs, self.device
        self.n_params = int(self.L.rx_ppo_n_params(venv.D))
        self.stride = (self.n_params + STRIDE_ALIGN - 1) // STRIDE_ALIGN * STRIDE_ALIGN
        self.params = torch.zeros((self.pool_size, self.stride), dtype=torch.float32, device=dev)
        self.log_std = torch.zeros((self.pool_size, 2), dtype=torch.float32, device=dev)
        self.opp_id = torch.zeros(n, dtype=torch.int32, device=dev)
        self.draw_count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.tally = torch.zeros((self.pool_size, _lib.RX_LEAGUE_TALLY_W), dtype=torch.int64, device=dev)
        self.cdf = torch.ones(self.pool_size, dtype=torch.float64, device=dev)
        self.n_live = 0
        self._opp_eps = torch.empty((n, 2), dtype=torch.float32, device=dev)
        self._sink = torch.empty((2, n), dtype=torch.float32, device=dev)
        # every address is fixed for the env's lifetime: one struct serves every call and any captured graph
        self.lg = _lib.RxLeagueIO(self.pool_size, self.agent_idx, _lib.ptr(self.params), _lib.ptr(self.log_std),
                                  self.stride, _lib.ptr(self.opp_id), _lib.ptr(self.draw_count),
                                  _lib.ptr(self.tally), _lib.ptr(self.cdf), self.seed, self.prec)
        ob = self.venv.buf["obs"][:, self.opp_idx]
        act = self._act[:, self.opp_idx]
        io = _lib.RxPolicyIO(venv.D, n, _lib.view_ptr(ob), _lib.ptr(self._opp_eps), _lib.ptr(self.params),
                             _lib.ptr(self.log_std), _lib.view_ptr(act), _lib.ptr(self._sink[0]),
                             _lib.ptr(self._sink[1]), ob.stride(0), act.stride(0), self.prec, None, 0)
        self._bank_io = _lib.RxPolicyBankIO(io, self.pool_size, 1, self.stride, _lib.ptr(self.opp_id))

    def set_opponent(self, policy, flat=None, prec=0):
        if policy is not None:
            raise ValueError("LeagueVectorEnv draws its opponents from the bank: use set_slot / weights / draw_all")
        super().set_opponent(None)

    def set_slot(self, k, agent, reset_tally=True):
        """Copy ``agent`` (a module of the reference layout) into bank slot k; a
        slot that held another snapshot starts its tally again."""
        if not 0 <= int(k) < self.pool_size:
            raise ValueError(f"slot {k} outside 0..{self.pool_size - 1}")
        flat = flat_policy_copy(agent)
        if flat.numel() != self.n_params or flat.dtype != torch.float32:
            raise ValueError(f"slot {k}: the policy has {flat.numel()} {flat.dtype} parameters, the bank's layout "
                             f"has {self.n_params} float32")
        with torch.no_grad():
            self.params[k, :self.n_params].copy_(flat)
            self.log_std[k].copy_(agent.log_std.detach().reshape(2))
            if reset_tally:
                self.tally[k].zero_()

    def weights(self, n_live, power=1, mix=0.1, prior=1.0, stream=None):
        """tallies -> sampling table over slots 0 .. n_live - 1 (rx_league_weights)."""
        _lib.check(self.L.rx_league_weights(ctypes.byref(self.lg), int(n_live), int(power), float(mix), float(prior),
                                            _lib.stream_ptr(stream)), "rx_league_weights")
        self.n_live = int(n_live)

    def clear(self):
        """No live slot: the random opponent, as SelfPlayPPO with an empty pool."""
        self.n_live = 0

    def draw_all(self, stream=None):
        """A fresh opponent for every env, nothing tallied (after the pool changed)."""
        _lib.check(self.L.rx_league_draw(ctypes.byref(self.lg), self.num_envs, None, None, _lib.stream_ptr(stream)),
                   "rx_league_draw")

    def _opponent_actions(self):
        if self.n_live == 0:
            return super()._opponent_actions()
        self._opp_eps.normal_()
        _lib.check(self.L.rx_policy_act_bank(ctypes.byref(self._bank_io), _lib.stream_ptr(None)),
                   "rx_policy_act_bank")

    def step_device(self, actions, obs_out=None, reward_out=None, done_out=None, **kw):
        kw["full_info"] = True
        o, r, done = super().step_device(actions, obs_out=obs_out, reward_out=reward_out, done_out=done_out, **kw)
        if self.n_live > 0:
            _lib.check(self.L.rx_league_draw(ctypes.byref(self.lg), self.num_envs, _lib.ptr(done),
                                             _lib.ptr(self.venv.buf["info"]), _lib.stream_ptr(kw.get("stream"))),
                       "rx_league_draw")
        return o, r, done


class LeagueStepRollout(SelfPlayStepRollout):
    """rx_league_rollout_steps driver: the two-car rollout loop with the opponents
    from the bank -- per step one policy launch (learner actor + critic, opponents
    through the bank), rx_step; the tally and redraw of a step runs inside the next
    step's policy launch, with one small launch after the last.  Every address
    handed to the library is fixed and nothing that changes between updates (the
    number of live slots, the table, the ids) is a by-value argument or part of the
    cache key, so a captured graph of the call stays valid while the pool fills."""

    FN = "rx_league_rollout_steps"

    @staticmethod
    def supported(lenv, agent, config):
        mode = config.get("rollout_steps", "auto")
        if mode is False or mode == "off":
            return False
        v = getattr(lenv, "venv", None)
        return (v is not None and hasattr(v, "_h") and hasattr(lenv, "lg") and lenv.n_live > 0 and v.n_agents == 2
                and policy_supported(agent, v.D))

    def _opponent(self):
        return None, None, 0  # the bank is in the league io: nothing of it in the struct or the cache key

    def _enqueue(self, args, stream):
        _lib.check(self.L.rx_league_rollout_steps(self.venv._h, self.venv._io_info(), *args,
                                                  ctypes.byref(self.spenv.lg), self.prec, stream), self.FN)


class LeagueSelfPlayPPO(SelfPlayPPO):
    """SelfPlayPPO whose rollout draws an opponent per env from the whole pool.

    The pool keeps the reference's cadence (``snapshot_freq``, FIFO of
    ``pool_size``) and ``opponent_pool`` stays the list of modules, oldest first;
    beside it snapshot number s is copied into bank slot s % pool_size (a reused
    slot's tally starts again).  Per update: advance_pool, the sampling table from
    the tallies (config ``pfsp_power`` = 1, ``pfsp_mix`` = 0.1, ``pfsp_prior`` =
    1.0), a fresh draw for every env, the env rebuild.  With an empty pool it is
    SelfPlayPPO: the random opponent on the per-step path.

    Refused (ValueError): pool_size > 64, a world size above 1 (per-rank tallies
    would need an all-reduce), a policy rx.ppo_fused.policy_supported
    refuses."""

    def __init__(self, env_fn, config, device="cuda"):
        self._slots = PoolSlots(config["pool_size"])  # refuses pool_size > 64
        if rdist.world() > 1:
            raise ValueError("LeagueSelfPlayPPO needs world size 1: the head-to-head tallies are per rank and the "
                             "sampling table would need their all-reduce")
        self.pfsp_power = int(config.get("pfsp_power", 1))
        self.pfsp_mix = float(config.get("pfsp_mix", 0.1))
        self.pfsp_prior = float(config.get("pfsp_prior", 1.0))
        if not 0 <= self.pfsp_power <= _lib.RX_LEAGUE_MAX_POWER:
            raise ValueError(f"pfsp_power={self.pfsp_power} outside 0..{_lib.RX_LEAGUE_MAX_POWER}")
        if not 0.0 <= self.pfsp_mix <= 1.0:
            raise ValueError(f"pfsp_mix={self.pfsp_mix} outside [0, 1]")
        if not self.pfsp_prior > 0.0:
            raise ValueError(f"pfsp_prior={self.pfsp_prior} must be > 0")
        super().__init__(env_fn, config, device)
        if not policy_supported(self.agent, self.envs.venv.D):
            raise ValueError("LeagueSelfPlayPPO: the policy does not have the reference actor-critic layout")

    def _make_venv(self, env_fn):
        """The reset two-car vector env of this trainer (SelfPlayPPO's)."""
        return super()._make_envs(env_fn).venv

    def _make_envs(self, env_fn):
        from . import ppo_fused
        c = self.config
        return LeagueVectorEnv(self._make_venv(env_fn), 0, seed=c["seed"] + rdist.rank(), pool_size=c["pool_size"],
                               prec=ppo_fused.precision(c))

    def advance_pool(self, update):
        """SelfPlayPPO's cadence; a new snapshot is also copied into its bank slot."""
        if update > 0 and update % self.snapshot_freq == 0:
            snap = self.snapshot_agent()
            self.opponent_pool.append(snap)
            if len(self.opponent_pool) > self.pool_size:
                self.opponent_pool.pop(0)
            _, slot, _ = self._slots.push()
            self.envs.set_slot(slot, snap, reset_tally=True)

    def update_opponent(self):
        """The sampling table from the tallies, a fresh opponent for every env, the env rebuild."""
        self.curr_opponent = None
        n_live = len(self.opponent_pool)
        if n_live == 0:
            self.envs.clear()
        else:
            self.envs.weights(n_live, self.pfsp_power, self.pfsp_mix, self.pfsp_prior)
            self.envs.draw_all()
        self._rebuild_envs()

    def collect_rollout(self, *bufs):
        # SelfPlayPPO's one captured graph per opponent kind; here the kind is random vs bank
        # (``envs.opponent_policy`` stays None: no module drives the opponent car)
        graphs = self.__dict__.setdefault("_graphs_by_kind", {})
        self._graphs = graphs.setdefault(self.envs.n_live > 0, {})
        return PPO.collect_rollout(self, *bufs)

    def _step_rollout(self, obs):
        from . import ppo_fused
        c = self.config
        if self._fused_policy(obs) is None or not LeagueStepRollout.supported(self.envs, self.agent, c):
            return None
        T, prec = obs.shape[0], ppo_fused.precision(c)
        sr = self.__dict__.get("_lg_steps_rollout")
        if sr is None or sr.T != T or sr.n != self.envs.num_envs or sr.prec != prec:
            sr = self._lg_steps_rollout = LeagueStepRollout(self.agent, self._flat, self.envs, T, prec)
        return sr

    def head_to_head(self):
        """The learner's record against every pool member, oldest first: one dict each
        (games, wins, losses, draws, the learner's win rate with a draw as half a win;
        None before the first game).  One device-to-host copy; call it between updates."""
        t = self.envs.tally.cpu().numpy()
        out = []
        for member, (s, slot) in enumerate(zip(self._slots.members(), self._slots.member_slots())):
            g, w, l = (int(v) for v in t[slot])
            out.append({"member": member, "snapshot": s, "slot": slot, "games": g, "wins": w, "losses": l,
                        "draws": g - w - l, "win_rate": (w + 0.5 * (g - w - l)) / g if g else None})
        return out

    def _checkpoint_extra(self):
        e = self.envs
        return {"league_state": {"n_snapshots": self._slots.n_snapshots, "slots": self._slots.member_slots(),
                                 "tally": e.tally.cpu(), "draw_count": e.draw_count.cpu(), "opp_id": e.opp_id.cpu()}}

    def _checkpoint_loaded(self, ck):
        """Rebuild the bank from the restored pool; a SelfPlayPPO checkpoint (no
        "league_state") numbers its pool 0, 1, ... with empty tallies."""
        ls = ck.get("league_state")
        n_pool = len(self.opponent_pool)
        if n_pool > self.pool_size:
            raise ValueError(f"the checkpoint's pool has {n_pool} members, pool_size is {self.pool_size}")
        self._slots = PoolSlots(self.pool_size, int(ls["n_snapshots"]) if ls else n_pool)
        slots = self._slots.member_slots()
        if ls and (list(ls["slots"]) != slots or tuple(ls["tally"].shape) != tuple(self.envs.tally.shape)):
            raise ValueError("the checkpoint's league_state does not fit this pool_size")
        e = self.envs
        e.tally.zero_()
        for slot, o in zip(slots, self.opponent_pool):
            e.set_slot(slot, o, reset_tally=False)
        if ls:
            e.tally.copy_(ls["tally"])
            if ls["draw_count"].numel() == e.num_envs:
                e.draw_count.copy_(ls["draw_count"])
                e.opp_id.copy_(ls["opp_id"])


def format_head_to_head(rows):
    lines = [f"{'member':>6} {'snapshot':>8} {'slot':>4} {'games':>8} {'wins':>8} {'losses':>8} {'draws':>8} "
             f"{'win rate':>8}"]
    for r in rows:
        wr = "-" if r["win_rate"] is None else f"{r['win_rate']:.3f}"
        lines.append(f"{r['member']:>6} {r['snapshot']:>8} {r['slot']:>4} {r['games']:>8} {r['wins']:>8} "
                     f"{r['losses']:>8} {r['draws']:>8} {wr:>8}")
    return "\n".join(lines)


__all__ = ["PoolSlots", "LeagueVectorEnv", "LeagueStepRollout", "LeagueSelfPlayPPO", "format_head_to_head"]
