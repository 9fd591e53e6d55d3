"""Helpers of tests/test_schedule_cpu.py and tests/test_sanitizers_cpu.py: the scenario file tests/cpp/schedule_main.cpp reads, its log, the
normalised dependency graph of a trace and the order rules checked on it."""
from collections import namedtuple

FLAGS = {"KEEP_TAPS": 1, "NO_PIPELINE": 2, "PLL_STREAM_ORDER": 32, "FAST_MATH": 64, "RDS_DECODE": 128}
CONTROLS = {"off": 0, "in_tile": 1, "serial": 2}        # no de-emphasis; 50 us (inside k_front's tile in the tolerance mode); 150 us (always a stage of its own)
DRAINS = ("synchronize", "reset", "set_output_lag", "controls", "pll_adaptive", "split_front")     # calls behind which every queue has run dry (controls: at the next block)
STAGES = ("predecim", "front", "deemph", "power", "pll", "extract", "rds")


def expand(calls):
    out = []
    for c in calls:
        if c[0] == "repeat":
            for _ in range(c[1]):
                out += expand(c[2])
        else:
            out.append(c)
    return out


def scenario_text(scenarios) -> str:
    lines = []
    for s in scenarios:
        lines.append(f"scenario {s['name']} {s['stations']} {s['block']} {s['fs']} {sum(FLAGS[f] for f in s['flags'])}")
        for c in expand(s["calls"]):
            args = [CONTROLS[c[1]]] if c[0] == "controls" else c[1:]
            lines.append(" ".join(map(str, [c[0], *args])))
        lines.append("end")
    return "\n".join(lines) + "\n"


def split_log(text: str) -> dict:
    """{scenario: [lines]} of a log: "== name" ... "== end"; lines outside are not part of any scenario."""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("== "):
            cur = None if line == "== end" else out.setdefault(line[3:], [])
        elif cur is not None and line.strip():
            cur.append(line.strip())
    return out


Op = namedtuple("Op", "what args waits")          # waits: frozenset of (queue, index in that queue's list)
Graph = namedtuple("Graph", "queues order calls")  # order: [(queue, index)] in host order; calls: per op the index of the call ("# ..." line) it was made in


def normalise(lines) -> Graph:
    queues, order, calls, carrier, pending, n_call = {}, [], [], {}, {}, -1
    for line in lines:
        if line.startswith("#"):
            n_call += 1
            continue
        w = line.split()
        if w[0] == "wait":
            if w[2] in carrier:
                pending.setdefault(w[1], set()).add(carrier[w[2]])
            continue
        if w[0] == "record":
            q, what, args, carried = w[2], "record", (w[1],), [w[1]]
        elif w[0] == "copy_hint":
            q, what, args, carried = w[1], "copy_hint", (), []
        else:
            assert w[0] == "launch", line
            kv = dict(x.split("=") for x in w[3:])
            q, what, args = w[2], "launch", (w[1], *(kv[k] for k in ("buf", "par", "seq", "warm", "t0", "t1", "done", "ride")))
            carried = [kv[k] for k in ("t1", "done") if kv[k] != "-"]
        node = (q, len(queues.setdefault(q, [])))
        queues[q].append(Op(what, args, frozenset(pending.pop(q, ()))))
        order.append(node)
        calls.append(n_call)
        for e in carried:
            carrier[e] = node
    for q, waits in sorted(pending.items()):
        queues.setdefault(q, []).append(Op("end", (), frozenset(waits)))
    return Graph(queues, order, calls)


def check_rules(scenario, lines) -> list:
    """The order rules, as happens-before in the normalised graph.  Edges: a queue's own order (the caller's streams count as one queue only where every stage
    runs on them: FMD_FLAG_NO_PIPELINE) and producer -> waiter.  Blocks on either side of a call that drains every queue (DRAINS) are ordered by the host and
    are not compared.  Returns the violations."""
    g = normalise(lines)
    fast, unpipelined = "FAST_MATH" in scenario["flags"], "NO_PIPELINE" in scenario["flags"]
    calls = expand(scenario["calls"])
    drain_epoch, reset_epoch, e, r = [], [], 0, 0
    for c in calls:
        e += c[0] in DRAINS
        r += c[0] == "reset"
        drain_epoch.append(e)
        reset_epoch.append(r)
    index = {node: i for i, node in enumerate(g.order)}
    before = []                                   # per op (host order): bit set of the ops that happen before it
    for i, (q, k) in enumerate(g.order):
        preds = [index[p] for p in g.queues[q][k].waits]
        if k > 0 and (q != "caller" or unpipelined):
            preds.append(index[(q, k - 1)])
        m = 0
        for p in preds:
            m |= before[p] | (1 << p)
        before.append(m)
    hb = lambda a, b: a is not None and b is not None and bool(before[b] >> a & 1)

    # the blocks: a front-end launch each; every other stage belongs to the newest front end with its buf (a first decimator: to the next one)
    blocks, by_buf, waiting_predecim = [], {}, {}
    for i, (q, k) in enumerate(g.order):
        op = g.queues[q][k]
        if op.what != "launch":
            continue
        stage, buf, seq, ride = op.args[0], int(op.args[1]), int(op.args[3]), op.args[8]
        if stage == "predecim":
            waiting_predecim[buf] = i
        elif stage == "front":
            b = {"front": i, "epoch": drain_epoch[g.calls[i]], "seq": 0}
            if buf in waiting_predecim:
                b["predecim"] = waiting_predecim.pop(buf)
            by_buf[buf] = b
            blocks.append(b)
            if ride != "-":
                by_buf[int(ride.split(",")[0])]["pll"] = i
        else:
            by_buf[buf][stage] = i
            if stage == "pll":
                by_buf[buf]["seq"] = seq
    bad = []
    for n, b in enumerate(blocks):
        prev = blocks[n - 1] if n and blocks[n - 1]["epoch"] == b["epoch"] else None
        for st in STAGES:
            # (a) the same stage of consecutive blocks runs in order (k_pilot_pll launches that hand over per wavefront: by their sequence numbers)
            if prev and st in prev and st in b:
                if st == "pll" and b["seq"] and prev["seq"]:
                    if b["seq"] != prev["seq"] + 1:
                        bad.append(f"(a) block {n}: pilot sequence number {b['seq']} behind {prev['seq']}")
                elif not hb(prev[st], b[st]):
                    bad.append(f"(a) block {n}: {st} not behind block {n - 1}'s")
        # (b) every stage follows its producer within the block
        fm_out = b.get("deemph", b["front"])
        for st, prod in (("front", b.get("predecim")), ("deemph", b["front"]), ("power", fm_out), ("pll", fm_out), ("extract", fm_out), ("extract", b.get("pll")), ("rds", b.get("extract"))):
            if st in b and prod is not None and b[st] != prod and not hb(prod, b[st]):
                bad.append(f"(b) block {n}: {st} not behind its producer")
        if "extract" in b and "pll" not in b:
            bad.append(f"(b) block {n}: extract stage without a pilot stage")
        # (c) the front end and the first decimator of block b follow the RDS stage of block b - 6
        if n >= 6 and blocks[n - 6]["epoch"] == b["epoch"]:
            for st in ("front", "predecim"):
                if st in b and not hb(blocks[n - 6].get("rds"), b[st]):
                    bad.append(f"(c) block {n}: {st} not behind block {n - 6}'s RDS stage")
        # (d) tolerance mode: the pilot stage of block b follows the extract stage of block b - 5, also when it rides a front end
        if fast and n >= 5 and blocks[n - 5]["epoch"] == b["epoch"] and "pll" in b and not hb(blocks[n - 5].get("extract"), b["pll"]):
            bad.append(f"(d) block {n}: pilot stage not behind block {n - 5}'s extract stage")
        # (f) the first front end after the last de-emphasised block follows that block's de-emphasis stage
        if prev and "deemph" in prev and "deemph" not in b and not hb(prev["deemph"], b["front"]):
            bad.append(f"(f) block {n}: front end not behind block {n - 1}'s de-emphasis stage")
    # (e) extract and RDS of a block follow the release event of that slot while a consumer holds it (until the slot's next block, or a reset)
    for i, (q, k) in enumerate(g.order):
        op = g.queues[q][k]
        if op.what == "record" and op.args[0].startswith("C"):
            for st in ("extract", "rds"):
                nxt = next((j for j in range(i + 1, len(g.order)) if g.queues[g.order[j][0]][g.order[j][1]].what == "launch" and
                            g.queues[g.order[j][0]][g.order[j][1]].args[:2] == (st, op.args[0][1:])), None)
                if nxt is not None and reset_epoch[g.calls[nxt]] == reset_epoch[g.calls[i]] and not hb(i, nxt):
                    bad.append(f"(e) {st} stage into slot {op.args[0][1:]} not behind its release")
    return bad
