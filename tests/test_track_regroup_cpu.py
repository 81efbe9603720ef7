"""Positions regrouped by slot without a GPU: the host twin rx_regroup_plan_host against a
NumPy restatement written here (np.argsort(pos_slot, kind="stable"), the gathers and the
inverse; integers throughout, so element for element), each of its refusals, the new
exports, and the trainer option's range check."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rx_regroup_plan_host", "rx_regroup_plan", "rx_regroup_slots", "rx_lane_layout")
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4200)
TRACKS = (1, 2, 200, 256, 257, 65537)
PATTERNS = ("one_slot", "grouped", "reversed", "random", "distinct", "sparse")
OUTS = ("src", "perm", "pos_slot", "env_pos")


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


# ---- the restatement and the cases (shared with tests/test_track_regroup_gpu.py) ---------------------
def py_regroup(perm, pos_slot):
    """-> dict(src, perm, pos_slot, env_pos): the positions in the stable order of their slots."""
    src = np.argsort(pos_slot, kind="stable").astype(np.int32)
    new_perm = perm[src]
    env_pos = np.empty(len(perm), dtype=np.int32)
    env_pos[new_perm] = np.arange(len(perm), dtype=np.int32)
    return dict(src=src, perm=new_perm, pos_slot=pos_slot[src], env_pos=env_pos)


def key_pattern(name, n, n_tracks, rs):
    """pos_slot int32 [n].  one_slot: every position on one slot; grouped / reversed: already in
    order, and in the opposite one; random; distinct: no slot twice where n_tracks >= n, else every
    slot in turn; sparse: the slots spread over the whole range, 0 and n_tracks - 1 among them
    (with n_tracks > n most slots stay empty and the top digit is in use)."""
    if name == "one_slot":
        k = np.full(n, n_tracks // 2)
    elif name in ("grouped", "reversed"):
        k = np.sort(rs.randint(0, n_tracks, size=n))
        k = k[::-1] if name == "reversed" else k
    elif name == "random":
        k = rs.randint(0, n_tracks, size=n)
    elif name == "distinct":
        k = rs.permutation(n_tracks)[:n] if n_tracks >= n else np.arange(n) % n_tracks
    else:
        k = rs.permutation(np.linspace(0, n_tracks - 1, num=n).round().astype(np.int64)) if n else np.zeros(0)
    return np.ascontiguousarray(k, dtype=np.int32)


def case(name, n, n_tracks):
    """-> (perm, pos_slot): a random env order and the pattern's slots, a function of the arguments alone."""
    rs = np.random.RandomState((1000003 * n + 31 * n_tracks + PATTERNS.index(name)) % 2 ** 32)
    return rs.permutation(n).astype(np.int32), key_pattern(name, n, n_tracks, rs)


def host_plan(L, n, n_tracks, perm, pos_slot, fill=-5):
    """One call of the twin -> (rc, dict of the four outputs, each pre-filled with ``fill``)."""
    from rx import _lib
    out = {k: np.full(max(n, 1), fill, dtype=np.int32) for k in OUTS}
    rc = L.rx_regroup_plan_host(n, n_tracks, _lib.ptr(perm), _lib.ptr(pos_slot), *(_lib.ptr(out[k]) for k in OUTS))
    return rc, {k: v[:max(n, 0)] for k, v in out.items()}


# ---- 1: exports ---------------------------------------------------------------------------------------
def test_the_new_exports_exist_and_the_abi_stays_25(L):
    import ctypes
    from rx import _lib
    assert L.rx_abi_version() == 25 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    for name in NEW:  # (the twin is declared int32_t, as rx_steps_plan is: it is no shared-body (device, host) pair)
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert f"int {name}(" in hdr or f"int32_t {name}(" in hdr, name
    name = "rx_regroup_scratch_bytes"
    assert hasattr(L, name) and name in _lib.EXPORTS and f"int64_t {name}(" in hdr
    assert L.rx_regroup_scratch_bytes.restype is ctypes.c_int64
    assert L.rx_regroup_scratch_bytes(-1, 4) == -1 and L.rx_regroup_scratch_bytes(4, 0) == -1
    for n in (0, 1, 256, 257, 70001):  # room for two index buffers and a 256-row count table at the least
        assert L.rx_regroup_scratch_bytes(n, 7) >= 4 * (2 * n + 256 * ((n + 255) // 256))


# ---- 2: the twin against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("n_tracks", TRACKS)
def test_plan_host_equals_the_restatement(L, n_tracks):
    for n in SIZES:
        for name in PATTERNS:
            perm, pos_slot = case(name, n, n_tracks)
            keep = perm.copy(), pos_slot.copy()
            rc, got = host_plan(L, n, n_tracks, perm, pos_slot)
            assert rc == 0, (n, name, L.rx_last_error())
            want = py_regroup(perm, pos_slot)
            for k in OUTS:
                assert got[k].tobytes() == want[k].tobytes(), (n, name, k)
            assert np.array_equal(perm, keep[0]) and np.array_equal(pos_slot, keep[1]), "the inputs are read only"
            if n:
                assert (np.diff(got["pos_slot"]) >= 0).all() and np.array_equal(got["env_pos"][got["perm"]],
                                                                                np.arange(n))


def test_the_cases_cover_what_they_claim():
    for n_tracks in TRACKS:
        for n in SIZES[2:]:
            k = {name: case(name, n, n_tracks)[1] for name in PATTERNS}
            assert len(set(k["one_slot"].tolist())) == 1
            assert (np.diff(k["grouped"]) >= 0).all() and (np.diff(k["reversed"]) <= 0).all()
            assert len(set(k["distinct"].tolist())) == min(n, n_tracks)
            assert k["sparse"].min() == 0 and k["sparse"].max() == n_tracks - 1
            for v in k.values():
                assert v.dtype == np.int32 and len(v) == n and v.min() >= 0 and v.max() < n_tracks
    assert case("sparse", 4200, 65537)[1].max() >> 16 == 1, "the third digit"
    assert not (np.diff(case("random", 257, 257)[1]) >= 0).all()


# ---- 3: refusals ----------------------------------------------------------------------------------------
def test_each_refusal_of_the_twin_has_its_own_message(L):
    from rx import _lib
    perm, pos_slot = case("random", 65, 7)

    def refused(n, n_tracks, p, s, null=None):
        out = {k: np.full(65, -5, dtype=np.int32) for k in OUTS}
        args = [_lib.ptr(p), _lib.ptr(s)] + [_lib.ptr(out[k]) for k in OUTS]
        if null is not None:
            args[null] = None
        rc = L.rx_regroup_plan_host(n, n_tracks, *args)
        assert rc == _lib.RX_EINVAL
        assert all((v == -5).all() for v in out.values()), "a refusal writes nothing"
        return L.rx_last_error().decode()

    seen = [refused(-1, 7, perm, pos_slot), refused(65, 0, perm, pos_slot), refused(65, -3, perm, pos_slot)]
    assert "n must be >= 0 (got -1)" in seen[0]
    assert "n_tracks must be > 0 (got 0)" in seen[1] and "(got -3)" in seen[2]
    for i, name in enumerate(("perm", "pos_slot", "src_out", "perm_out", "pos_slot_out", "env_pos_out")):
        msg = refused(65, 7, perm, pos_slot, null=i)
        assert msg.endswith(f"null {name}"), msg
        seen.append(msg)
    for at, k in ((0, -1), (64, 7), (30, 1 << 20)):
        bad = pos_slot.copy()
        bad[at] = k
        msg = refused(65, 7, perm, bad)
        assert f"pos_slot[{at}] = {k} outside [0, 7)" in msg
        seen.append(msg)
    bad = perm.copy()
    bad[3] = 65
    seen.append(refused(65, 7, bad, pos_slot))
    assert "perm[3] = 65" in seen[-1]
    assert len(set(seen)) == len(seen) and all(m.startswith("rx_regroup_plan_host: ") for m in seen)
    rc, got = host_plan(L, 65, 7, perm, pos_slot)  # ... and the same arrays, unharmed, are accepted
    assert rc == 0 and got["src"].tobytes() == py_regroup(perm, pos_slot)["src"].tobytes()


def test_the_device_entry_checks_its_arguments_before_any_launch(L):
    """rx_regroup_plan's refusals need no device: n, n_tracks, a null pointer, the scratch size."""
    from rx import _lib
    a = np.zeros(80, dtype=np.int32)
    p = _lib.ptr(a)
    need = L.rx_regroup_scratch_bytes(65, 7)
    for args, text in (((-1, 7) + (p,) * 7 + (need, None), "n must be >= 0"),
                       ((65, 0) + (p,) * 7 + (need, None), "n_tracks must be > 0"),
                       ((65, 7) + (p,) * 6 + (None, need, None), "null scratch"),
                       ((65, 7) + (p, None) + (p,) * 5 + (need, None), "null pos_slot"),
                       ((65, 7) + (p,) * 7 + (need - 1, None), f"scratch of {need - 1} bytes")):
        assert L.rx_regroup_plan(*args) == _lib.RX_EINVAL
        assert text in L.rx_last_error().decode(), L.rx_last_error()
    assert L.rx_regroup_slots(None, None) == _lib.RX_EINVAL and b"null handle" in L.rx_last_error()
    assert L.rx_lane_layout(None, p, p, p) == _lib.RX_EINVAL and b"null handle" in L.rx_last_error()


# ---- 4: the trainer option -------------------------------------------------------------------------------
def test_a_negative_regroup_cadence_is_refused_before_a_device_is_touched():
    from rx.configs import base_config
    from rx.track_episodic import EpisodicCurriculumPPO
    from rx.track_replay_episodic import EpisodicReplayCurriculumPPO
    for cls in (EpisodicCurriculumPPO, EpisodicReplayCurriculumPPO):
        with pytest.raises(ValueError, match="episodic_regroup_every=-1"):
            cls(lambda i: None, base_config(num_envs=64, num_steps=16, episodic_regroup_every=-1))
