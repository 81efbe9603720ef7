"""rx_steps_plan: the launch schedule of an rx_steps call as a pure function (include/rx.h,
DESIGN.md §3 "The deep launch"), checked by brute force without a GPU.

Every plan of the grid -- K in 1..40 and 67, depth 2 / 4 / 8, sort_interval 0 / 1 / 2 / 3 / 8
at every starting dyn_calls phase, task_sort 1 / 2 / 3 at every task_calls phase, both
tasks_stale values, with and without crossing, and the lag-1 schedule (rank_in_kin) at depth
2 -- is replayed on a clock (launch i at time 2 i, the sort and the k_kin1 behind it at
2 i + 1) and held to the rules the kernels rely on:

* every step has one REWARD, in order, its KIN before it, and one ray cast;
* the ranked steps are those of K x rx_step's cadence, each ranked once, in a launch strictly
  after its KIN's and strictly before its rays' (lag 1: by its own KIN);
* a ray step reads the row of the last ranked step up to it (the handle's buffer when the
  call has ranked none), written strictly earlier;
* no ring slot (pose, task row, crossing snapshot) is written while a reader still needs it,
  none is read and written in one launch, and the slots are inside their rings;
* the key-writing REWARD is a re-sort step's, last in its launch, the sort follows it and the
  next KIN is a k_kin1 behind the sort; a step cast after the sort that closed its window
  reads that sort's snapshot, any other the live rows; without crossing no step is queued
  across a sort;
* the ray steps of a launch are in step order on distinct obs targets, the newest on the
  caller's rows, and steps are cast in order over the call, so the rows end with step K - 1's;
* the queues are empty at the end and the counts are K x rx_step's.
"""
import pytest

KS = list(range(1, 41)) + [67]
INTERVALS = (0, 1, 2, 3, 8)


def _cadence(K, si, d0, ts, t0, stale):
    """Which steps K x rx_step ranks (their KIN parts take the turns, in step order; every
    re-sort marks the order stale), and tasks_stale after the last step."""
    ranked = []
    for s in range(K):
        if ts:
            r = stale or t0 % ts == 0
            t0 += 1
            if r:
                stale = False
            ranked.append(r)
        else:
            ranked.append(False)
        if si and (d0 + s) % si == 0:
            stale = True
    return ranked, stale


def _check(recs, ranked_out, stale_out, K, depth, si, d0, ts, t0, stale, cross, lag1):
    want_ranked, stale_end = _cadence(K, si, d0, ts, t0, stale)
    resort = [bool(si) and (d0 + s) % si == 0 for s in range(K)]
    P, T, C = 3 * depth, 2 * depth + 1, 3
    kin_t, kin_pose, rew_t, rank_t, ray_t = {}, {}, {}, {}, {}
    row_of, row_written = {}, {}     # step -> (slot it is ranked into), time of that write
    ray_row, ray_snap = {}, {}
    snaps = []                        # (time written, slot, re-sort step)
    sorts = []                        # (time, re-sort step)
    cast_order = []

    def do_kin(s, t, pose, row):
        assert s not in kin_t and 0 <= pose < P, (s, pose)
        kin_t[s], kin_pose[s] = t, pose
        if lag1:
            assert (row >= 0) == want_ranked[s], (s, row)
            if row >= 0:
                row_of[s], row_written[s] = row, t
        else:
            assert row == -1

    assert recs[0]["n_sub"] == recs[0]["n_rank"] == recs[0]["n_rays"] == 0 and recs[0]["kin1_after"] == 0
    next_reward = 0
    for i, L in enumerate(recs):
        t = 2 * i
        ns, nk, nr = L["n_sub"], L["n_rank"], L["n_rays"]
        assert 0 <= ns <= depth and 0 <= nk <= depth and 0 <= nr <= depth
        assert i == 0 or ns + nk + nr > 0
        assert lag1 <= (nk == 0)
        for j in range(ns):
            s = L["first_step"] + j
            assert s == next_reward and s in kin_t and kin_t[s] < t + (j > 0), s  # in order, KIN before it
            if j:
                assert L["kin"][j - 1] == 1 and kin_t[s] == t  # the chain: its KIN is the part before it
            rew_t[s] = t
            next_reward += 1
            if L["kin"][j]:
                assert s + 1 < K and not resort[s] and j + 1 <= depth
                do_kin(s + 1, t, L["kin_pose"][j], L["kin_row"][j])
            else:
                assert j == ns - 1  # a KIN-less REWARD ends the chain
            assert resort[s] <= (j == ns - 1)
        last = L["first_step"] + ns - 1 if ns else None
        keyed = ns > 0 and resort[last]
        assert L["keys"] == int(keyed) and L["sort_after"] == int(keyed)
        if keyed:
            assert not L["kin"][ns - 1]
            sorts.append((t + 1, last))
            if L["keys_snap"] >= 0:
                assert cross and L["keys_snap"] < C
                snaps.append((t, L["keys_snap"], last))
        else:
            assert L["keys_snap"] == -1
        for q in range(nk):
            s = L["rank_step"][q]
            assert s not in rank_t and want_ranked[s] and kin_t[s] < t and L["rank_pose"][q] == kin_pose[s]
            assert 0 <= L["rank_row"][q] < T
            rank_t[s], row_of[s], row_written[s] = t, L["rank_row"][q], t
        steps = [L["ray_step"][r] for r in range(nr)]
        assert steps == sorted(set(steps))
        shadows = [L["ray_shadow"][r] for r in range(nr)]
        if nr:
            assert shadows[-1] == -1 and len(set(shadows)) == nr and all(0 <= x < depth - 1 for x in shadows[:-1])
        for r, s in enumerate(steps):
            assert s not in ray_t and kin_t[s] < t and L["ray_pose"][r] == kin_pose[s]
            ray_t[s], ray_row[s], ray_snap[s] = t, L["ray_row"][r], L["ray_snap"][r]
            cast_order.append(s)
        if L["kin1_after"] >= 0:
            s = L["kin1_after"]
            assert i == 0 or (ns and not L["kin"][ns - 1] and s == last + 1)
            do_kin(s, t + 1, L["kin1_pose"], L["kin1_row"])
        elif ns and not L["kin"][ns - 1]:
            assert last == K - 1
    # every step once, queues empty, the counts of K x rx_step
    assert next_reward == K and sorted(kin_t) == sorted(ray_t) == list(range(K))
    assert cast_order == list(range(K))
    assert sum(L["n_sub"] for L in recs) == K
    assert ranked_out == sum(want_ranked) and stale_out == (stale_end or ranked_out > 0)
    if not lag1:
        assert sorted(rank_t) == [s for s in range(K) if want_ranked[s]]
    for s in rank_t:
        assert kin_t[s] < rank_t[s] < ray_t[s], s
    # a ray step's row: the last ranked step's up to it, written strictly earlier
    src = None
    readers = {}
    for s in range(K):
        if want_ranked[s]:
            src = s
        if src is None:
            assert ray_row[s] == -1, s
        else:
            assert ray_row[s] == row_of[src] and row_written[src] < ray_t[s], (s, src)
            readers.setdefault(src, []).append(ray_t[s])

    def ring(uses):
        """uses: (slot, time written, time of the last read); no slot is rewritten at or before the last
        read of what it held."""
        by = {}
        for slot, w, rd in uses:
            by.setdefault(slot, []).append((w, rd))
        for slot, v in by.items():
            v.sort()
            for (w0, r0), (w1, _) in zip(v, v[1:]):
                assert w1 > r0 >= w0, (slot, w0, r0, w1)

    ring([(kin_pose[s], kin_t[s], ray_t[s]) for s in range(K)])
    ring([(row_of[s], row_written[s], max(readers[s])) for s in row_of])
    # crossing snapshots: a step cast after the sort that closed its window reads that sort's
    snap_reads = {}
    for s in range(K):
        closing = next(((ts_, m) for ts_, m in sorts if m >= s), None)
        if closing is None or ray_t[s] < closing[0]:
            assert ray_snap[s] == -1, s
            continue
        assert cross, "a step queued across a sort without crossing"
        inst = [x for x in snaps if x[2] == closing[1]]
        assert len(inst) == 1 and ray_snap[s] == inst[0][1] and inst[0][0] < ray_t[s], s
        snap_reads.setdefault(inst[0], []).append(ray_t[s])
    ring([(slot, w, max(snap_reads.get((w, slot, m), [w]))) for w, slot, m in snaps])


def _grid(lag1):
    for depth in ((2,) if lag1 else (2, 4, 8)):
        for si in INTERVALS:
            for d0 in range(max(si, 1)):
                for ts in (1, 2, 3):
                    for t0 in range(ts):
                        for stale in (False, True):
                            for cross in (True, False):
                                yield depth, si, d0, ts, t0, stale, cross


@pytest.mark.parametrize("lag1", [False, True], ids=["deep", "lag1"])
def test_every_plan_of_the_grid(lag1):
    from rx import _lib
    n = launches = 0
    for depth, si, d0, ts, t0, stale, cross in _grid(lag1):
        for K in KS:
            recs, ranked, stale_out = _lib.steps_plan(K, depth, si, d0, ts, t0, stale, cross, lag1)
            try:
                _check(recs, ranked, stale_out, K, depth, si, d0, ts, t0, stale, cross, lag1)
            except AssertionError as e:
                raise AssertionError(f"K={K} depth={depth} si={si} d0={d0} ts={ts} t0={t0} stale={stale} "
                                     f"cross={cross} lag1={lag1}: {e!r}") from e
            n += 1
            launches += len(recs) - 1
    print(f"{n} plans, {launches} launches")


def test_a_handle_that_ranks_nothing():
    """task_sort 0 (lane-varying slots, ray orders without a task buffer): no RANK class, no row,
    and a step's rays follow its KIN by one launch."""
    from rx import _lib
    for depth in (2, 4, 8):
        for si in INTERVALS:
            for K in (1, 2, 9, 40):
                recs, ranked, _ = _lib.steps_plan(K, depth, si, 0, 0, 0, True, True, False)
                assert ranked == 0 and all(L["n_rank"] == 0 for L in recs)
                _check(recs, ranked, _, K, depth, si, 0, 0, 0, True, True, False)


def test_steady_state_and_the_parent_schedule():
    """Depth 4 without re-sorts: k_kin1(0), then [4 sub-steps | rank 4 | rays 4] once the queues
    have filled, and two drain launches.  The lag-1 plan of 20 steps from a re-sort step at
    sort_interval 8 is the paired schedule: k_kin1, [D0 D1 | rays 0], ..., [D6 R7 | 5 6], sort,
    k_kin1(8), [D8 D9 | 7 8], ... and the last step beside its own rays."""
    from rx import _lib
    recs, _, _ = _lib.steps_plan(40, 4, 0, 0, 1, 0, True, True, False)
    shape = [(L["n_sub"], L["n_rank"], L["n_rays"]) for L in recs]
    assert shape[:4] == [(0, 0, 0), (4, 1, 0), (4, 4, 1), (4, 4, 4)] and shape[-2:] == [(0, 3, 4), (0, 0, 3)]
    assert all(x == (4, 4, 4) for x in shape[3:10]) and len(recs) == 1 + 10 + 2
    recs, _, _ = _lib.steps_plan(20, 2, 8, 1, 1, 0, True, True, True)
    shape = [(L["n_sub"], L["n_rays"], L["keys"], L["kin1_after"]) for L in recs]
    assert shape == [(0, 0, 0, 0), (2, 1, 0, -1), (2, 2, 0, -1), (2, 2, 0, -1), (2, 2, 1, 8), (2, 2, 0, -1),
                     (2, 2, 0, -1), (2, 2, 0, -1), (2, 2, 1, 16), (2, 2, 0, -1), (1, 2, 0, -1), (1, 1, 0, -1)]


def test_bad_arguments():
    from rx import _lib
    for kw in (dict(n_steps=0), dict(depth=1), dict(depth=9), dict(sort_interval=-1), dict(task_sort=-1)):
        a = dict(n_steps=5, depth=2, sort_interval=8, dyn_calls=0, task_sort=1, task_calls=0)
        a.update(kw)
        with pytest.raises(_lib.RxError):
            _lib.steps_plan(**a)
