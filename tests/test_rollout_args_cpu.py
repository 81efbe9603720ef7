"""The argument checks of the five rollout drivers (rx.ppo_fused.Rollout, StepRollout,
SelfPlayStepRollout, rx.curriculum.CurriculumStepRollout, rx.league_train.LeagueStepRollout)
without a device: every refusal below is a ValueError raised before any library call, on CPU
tensors, with stubs for the env (only num_envs, D, buf are read before the checks)."""
from types import SimpleNamespace as NS

import pytest
import torch

T, N, D = 2, 3, 19
BUFFERS = ("obs", "actions", "logprobs", "dones", "rewards", "values", "next_obs", "next_done")
SHAPES = {"obs": (T, N, D), "actions": (T, N, 2), "logprobs": (T, N), "dones": (T, N), "rewards": (T, N),
          "values": (T, N), "next_obs": (N, D), "next_done": (N,)}
DRIVERS = ("Rollout", "StepRollout", "SelfPlayStepRollout", "CurriculumStepRollout", "LeagueStepRollout")
TWO_CAR = ("SelfPlayStepRollout", "LeagueStepRollout")


def _policy():
    return NS(log_std=torch.zeros(2)), NS(flat_param=torch.zeros(64))


def _driver(name):
    from rx import curriculum, league_train, ppo_fused
    agent, flat = _policy()
    venv = NS(num_envs=N, D=D, n_agents=2 if name in TWO_CAR else 1,
              buf={"obs": torch.zeros((N, 2, D)), "reward": torch.zeros((N, 2))})
    if name in TWO_CAR:
        oa, of = _policy()
        spenv = NS(venv=venv, agent_idx=0, _act=torch.zeros((N, 2, 2)), _opp_fused=NS(agent=oa, flat=of, prec=0), lg=None)
        cls = ppo_fused.SelfPlayStepRollout if name == "SelfPlayStepRollout" else league_train.LeagueStepRollout
        return cls(agent, flat, spenv, T)
    if name == "CurriculumStepRollout":
        return curriculum.CurriculumStepRollout(agent, flat, venv, T, NS(tc=None))
    return getattr(ppo_fused, name)(agent, flat, venv, T)


def _bufs(**over):
    b = {k: torch.zeros(SHAPES[k]) for k in BUFFERS}
    b.update(over)
    return [b[k] for k in BUFFERS]


@pytest.mark.parametrize("name", DRIVERS)
def test_a_wrong_buffer_is_refused_by_name(name):
    drv = _driver(name)
    for k in BUFFERS:
        with pytest.raises(ValueError, match=rf"\b{k}\b"):
            drv(*_bufs(**{k: torch.zeros(SHAPES[k] + (2,))}))
    with pytest.raises(ValueError, match=r"\bobs\b"):
        drv(*_bufs(obs=torch.zeros(SHAPES["obs"], dtype=torch.float64)))
    strided = torch.zeros((T, N, 4))[..., :2]
    assert tuple(strided.shape) == SHAPES["actions"] and not strided.is_contiguous()
    with pytest.raises(ValueError, match=r"\bactions\b"):
        drv(*_bufs(actions=strided))


@pytest.mark.parametrize("name", DRIVERS)
def test_a_wrong_shape_eps_is_refused(name):
    with pytest.raises(ValueError):
        _driver(name)(*_bufs(), eps=torch.zeros((T, N + 1, 2)))


@pytest.mark.parametrize("name", TWO_CAR)
def test_a_wrong_shape_opp_eps_is_refused(name):
    with pytest.raises(ValueError):
        _driver(name)(*_bufs(), opp_eps=torch.zeros((T, N, 3)))
