"""CPU: the model of tsw_task_timeline (tests/timeline_model.py) against itself. forward is online_model's loop
with a task log; replay reads the records alone. The records determine the timeline: on every case replay's
table equals forward's log, and tampered records are caught at the expected kind, column and agent with exactly
the earlier events kept."""
import numpy as np
import pytest

import timeline_model as tm
from online_model import online_mapd
from p2p_distributed_tswap_amd import maps

CPU_CASES = tm.CASES


@pytest.mark.parametrize("name", ["plain", "paced", "random-release", "ties"])
def test_forward_records_equal_the_online_model(name):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case(name)
    ref = online_mapd(maps.rows_to_array(rows), starts, tasks, rel, max_t)
    assert rec.shape == ref[0].shape and np.array_equal(rec, ref[0])


@pytest.mark.parametrize("name", CPU_CASES)
def test_replay_of_the_records_equals_the_forward_log(name):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case(name)
    got = tm.replay(rec, starts, tasks, rel)
    tm.assert_equal(got, tm.expected(name), name)
    assert got["consistent"] == 1 and got["assigned"] >= 1


def test_cases_exercise_what_they_are_for():
    c = {name: tm.case(name)[7] for name in ("plain", "ties", "busy", "scan-65-staggered")}
    assert c["ties"]["ties"] > 0
    assert c["busy"]["handovers"] > 0 and c["busy"]["multi_take"] > 0
    assert c["scan-65-staggered"]["half_dead"] > 0
    e = tm.expected("random-release")
    assert e["unreleased"] == 2 and e["delivered"] >= 1 and e["wait_sum"] > 0
    assert tm.expected("fewer-tasks")["assigned"] == 6


def test_a_column_prefix_keeps_open_tasks_open():
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("random-release")
    T = 40
    got = tm.replay(rec[:, :T], starts, tasks, rel)
    full = log.astype(np.int64)
    want = np.where((full != tm.NONE) & (full < T), full, tm.NONE)
    want[:, 0] = np.where(want[:, 1] != tm.NONE, full[:, 0], tm.NONE)
    assert np.array_equal(got["task"], want.astype(np.uint32)) and got["consistent"] == 1
    assert got["assigned"] > got["delivered"] and got["unreleased"] == np.count_nonzero(rel > T - 1)


@pytest.mark.parametrize("name", ["plain", "random-release", "fewer-tasks"])
def test_tampered_records(name):
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case(name)
    T = rec.shape[1]
    tampers = [tm.tamper_picking_to_idle(rec), tm.tamper_take_to_stay(rec, log)]
    if name != "fewer-tasks":
        tampers.append(tm.tamper_take_to_stay(rec, log, 5))  # (a hand-over in "plain": D -> I with a task to be had)
    if name != "plain":
        tampers.append(tm.tamper_idle_to_picking(rec, log, rel))
    kinds = set()
    for bad, kind, t, i in tampers:
        got = tm.replay(bad, starts, tasks, rel)
        assert (got["bad_kind"], got["bad_t"], got["bad_agent"]) == (kind, t, i)
        tm.assert_equal(got, tm.truncated(log, rel, T, kind, t, i), f"{name} kind {kind}")
        kinds.add(kind)
    assert kinds >= {0, 2}


def test_bad_state_is_kind_0():
    rows, starts, tasks, rel, max_t, rec, log, cnt = tm.case("plain")
    bad = tm._with_state(rec, 4, 9, 7)
    got = tm.replay(bad, starts, tasks, rel)
    tm.assert_equal(got, tm.truncated(log, rel, rec.shape[1], 0, 9, 4))


def test_stream_rule_on_a_hand_made_run():
    # two agents, three tasks: agent 0 takes 0 then 2, agent 1 takes 1; columns: I/P/C/D coded by hand
    P, C, D, I = tm.PICKING, tm.CARRYING, tm.DELIVERED, tm.ST_IDLE
    st = np.array([[P, P, C, D, P, C, D, I], [P, C, C, C, D, I, I, I]], dtype=np.uint64)
    rec = st << np.uint64(32)
    tasks = np.zeros((3, 4), dtype=np.uint32)
    got = tm.replay(rec, None, tasks, None, "stream")
    assert got["task"].tolist() == [[0, 0, 2, 3], [1, 0, 1, 4], [0, 4, 5, 6]] and got["consistent"] == 1
    assert got["makespan"] == 6 and got["service_sum"] == 13 and got["carry_sum"] == 1 + 3 + 1
    # a fourth task nobody takes: agent 0 stays idle at column 7 with the stream not empty
    got = tm.replay(rec, None, np.zeros((4, 4), dtype=np.uint32), None, "stream")
    assert (got["bad_kind"], got["bad_t"], got["bad_agent"]) == (2, 5, 1) and got["delivered"] == 2
