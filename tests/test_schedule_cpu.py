"""CPU-only: the block schedule (fm-radio_amd/csrc/fmd_schedule.cpp, built with plain g++ into tests/cpp/schedule_main.cpp and driven by a backend that
prints) against tests/golden/schedule_traces.json — the queue calls recorded from the code the unit replaced (how: the file's "about"; process_dev, launch_deferred,
launch_deferred_pll, outputs_wanted, sync_all while they were part of fmd_api.cpp, with a line printed at every hipStreamWaitEvent, hipEventRecord,
launch_stage_* and hint copy) for the same scenarios — and against the order rules the schedule exists to keep.

The one normalisation (schedule_graph.normalise): every wait is resolved to the launch or record that last carried its event in host order (a wait on an
event nothing has carried yet is dropped); per queue the trace is then the ordered list of launches, records and copies, each with its arguments — stage,
buf, par, seq, warm, ride, the events riding on the packet — and the set of producers it waits for; the waits a queue is left with at the end count as one
more entry.  Two traces are equal when these lists are.  So the waits in front of one operation may be issued in another host order; nothing else may differ."""
import json
import subprocess
from pathlib import Path

import pytest

import schedule_graph as G

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "schedule_traces.json").read_text())
NAMES = [s["name"] for s in GOLDEN["scenarios"]]


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("schedule")
    exe = tmp / "schedule_main"
    csrc = ROOT / "fm-radio_amd" / "csrc"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", f"-I{csrc}", str(ROOT / "tests" / "cpp" / "schedule_main.cpp"),
                        str(csrc / "fmd_schedule.cpp"), str(csrc / "fmd_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    (tmp / "scenarios.txt").write_text(G.scenario_text(GOLDEN["scenarios"]))
    r = subprocess.run([str(exe), str(tmp / "scenarios.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return G.split_log(r.stdout)


def test_the_scenarios_take_what_the_issue_lists():
    """What the scenarios must cover between them, as far as it shows in the recorded traces themselves."""
    by = {s["name"]: s for s in GOLDEN["scenarios"]}
    assert set(GOLDEN["traces"]) == set(NAMES) and len(NAMES) == len(set(NAMES)) >= 25
    text = {n: "\n".join(GOLDEN["traces"][n]) for n in NAMES}
    assert "seq=9" in text["exact_chained_process"] and "launch pll own" in text["exact_chained_process"] and "launch pll B" in text["exact_chained_process"]
    assert all(l.split()[2] == "caller" for l in GOLDEN["traces"]["exact_no_pipeline"] if l.startswith("launch")) and "done=-" in text["exact_no_pipeline"]
    assert "launch predecim F" in text["exact_1024k"] and "launch predecim own" in text["exact_1024k_stream_order"]
    assert text["exact_adaptive_moved_thresholds"].count("copy_hint A") >= 4
    assert "launch deemph D" in text["exact_deemph_on_and_off"] and "launch deemph D" in text["fast_deemph_serial"] and "launch deemph" not in text["fast_deemph_in_tile"]
    for n in ("fast_deferred_no_stream", "fast_deferred_ready_stream", "fast_deferred_lag_consumer", "fast_1024k_two_queues", "profile1_deferred"):
        assert "launch extract F" in text[n] and "ride=-" in text[n] and any("launch front" in l and "ride=-" not in l for l in GOLDEN["traces"][n]), n
    assert "launch front own" in text["fast_1024k_two_queues"] and "launch predecim own" in text["fast_1024k_split_front"]
    assert "launch extract F" in text["fast_keep_taps"] and all("ride=-" in l for l in GOLDEN["traces"]["fast_keep_taps"] if l.startswith("launch"))
    assert "launch extract X" in text["fast_deferred_wait_after_third"] and "launch extract F" in text["fast_deferred_wait_after_third"]
    assert any(" C" in l and l.startswith("wait") for l in GOLDEN["traces"]["fast_deferred_lag_consumer"])
    for m in (1, 2, 3):
        assert "t1:pll:" in text[f"profile{m}_exact"] and "t1:extract:" in text[f"profile{m}_deferred"]
    assert {c[0] for s in by.values() for c in G.expand(s["calls"])} >= {"process", "submit", "wait_outputs", "release_outputs", "wait_input", "synchronize", "reset",
                                                                          "set_output_lag", "controls", "profile", "pll_adaptive", "split_front"}


def test_the_run_has_the_golden_s_scenarios_and_no_others(traces):
    assert sorted(traces) == sorted(GOLDEN["traces"]) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_same_dependency_graph_as_the_code_it_replaced(traces, name):
    got, want = G.normalise(traces[name]), G.normalise(GOLDEN["traces"][name])
    assert sorted(got.queues) == sorted(want.queues), name
    for q in want.queues:
        for i, (g, w) in enumerate(zip(got.queues[q], want.queues[q])):
            assert g == w, f"{name}: queue {q}, entry {i}:\n  now    {g}\n  before {w}"
        assert len(got.queues[q]) == len(want.queues[q]), (name, q)


# Rules that do not hold in the recorded graphs: findings about the code the unit replaced, kept as they are (the unit reproduces its graph), to be fixed on their own.
#  * fast_1024k_split_front, rule (a): fmd_process_* followed by fmd_submit_* without a ready stream on a deferred-capable handle at 1.024 MSa/s.  The submitted block's
#    front end goes on the capture's queue (own), the processed block's went on F, and nothing orders the two (the front end carries its input history from
#    block to block).  The other way round the put-off block's extract stage, queued on F ahead of the processed block, happens to order them.
KNOWN = {"fast_1024k_split_front": {"(a) block 12: front not behind block 11's"}}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("which", ["new", "golden"])
def test_order_rules(traces, name, which):
    """Happens-before (a queue's own order, and producer -> waiter) in the normalised graph, for the rules the schedule's comments state: schedule_graph.check_rules."""
    sc = next(s for s in GOLDEN["scenarios"] if s["name"] == name)
    problems = G.check_rules(sc, traces[name] if which == "new" else GOLDEN["traces"][name])
    assert set(problems) == KNOWN.get(name, set()), f"{name} ({which}): " + "; ".join(problems[:5])


def test_the_rules_notice_a_missing_wait():
    """Each rule against a recorded trace with the waits that keep it taken out."""
    sc = next(s for s in GOLDEN["scenarios"] if s["name"] == "fast_small_process")
    lines = GOLDEN["traces"]["fast_small_process"]
    assert not G.check_rules(sc, lines)
    for rule, prefixes in (("(b)", ("wait R E",)), ("(c)", ("wait F X",)), ("(d)", ("wait B E",)), ("(e)", ("wait X C", "wait R C"))):
        cut = [l for l in lines if not l.startswith(prefixes)]
        assert len(cut) < len(lines) and any(p.startswith(rule) for p in G.check_rules(sc, cut)), rule
    sc = next(s for s in GOLDEN["scenarios"] if s["name"] == "exact_deemph_on_and_off")
    lines = GOLDEN["traces"]["exact_deemph_on_and_off"]
    cut = [l for l in lines if not l.startswith("wait F F")]
    assert len(cut) < len(lines) and any(p.startswith("(f)") for p in G.check_rules(sc, cut))
    sc = next(s for s in GOLDEN["scenarios"] if s["name"] == "fast_deferred_wait_after_third")       # (the extract stage changes queue there)
    lines = GOLDEN["traces"]["fast_deferred_wait_after_third"]
    cut = [l for l in lines if not l.startswith("wait X E")]
    assert len(cut) < len(lines) and any(p.startswith("(a)") for p in G.check_rules(sc, cut))
