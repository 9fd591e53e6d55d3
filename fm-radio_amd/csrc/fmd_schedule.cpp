// The rules of fmd_schedule.h.  Host only.
#include "fmd_schedule.h"

namespace fmd {

namespace {
Event slot_event(EventKind k, int slot) { Event e; e.kind = k; e.slot = slot; return e; }
Event timing_event(EventKind k, Stage st, int prof_block) { Event e; e.kind = k; e.stage = (unsigned char)st; e.slot = prof_block; return e; }
}  // namespace

#define SCHED_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

int Schedule::wait(ScheduleBackend& be, Queue q, Event e) {
    const int rc = be.wait(q, e);
    if (rc) failed_ = "hipStreamWaitEvent";
    return rc;
}

int Schedule::record(ScheduleBackend& be, Event e, Queue q) {
    const int rc = be.record(e, q);
    if (rc) failed_ = "hipEventRecord";
    return rc;
}

// Event bracketing perturbs the pipeline it measures (extra queue packets between dependent kernels): mode 2 keeps it on the dominant kernel and
// samples the others; mode 3 samples: every stage of every 4th block, plus the pilot stage of the block behind it (for the hand-over gap)
bool Schedule::timed(const Block& b, Stage st) const {
    if (b.prof_block < 0) return false;
    if (b.prof_mode == 3) return (b.block & 3) == 0 || (st == ST_PLL && (b.block & 3) == 1);
    return b.prof_mode == 1 || st == ST_PLL || (b.block & 3) == 0;
}

// One stage of block b on queue `on`: the timing events or else `done` ride on the stage's last dispatch packet; *dep is the event the next stage waits on.
int Schedule::run(ScheduleBackend& be, Stage st, Queue on, const Block& b, Event done, Event* dep, unsigned seq, const Launch* ride) {
    Launch l;
    l.buf = b.slot; l.par = b.par; l.seq = seq; l.warm = b.warm;
    if (timed(b, st)) { l.t0 = timing_event(EV_T0, st, b.prof_block); l.t1 = timing_event(EV_T1, st, b.prof_block); }
    if (cfg_.pipelined && !l.t1) l.done = done;
    *dep = l.t1 ? l.t1 : done;
    int rc = 0;
    if (cfg_.debug_skip & (1u << st)) rc = cfg_.pipelined ? be.record(*dep, on) : 0;
    else rc = be.launch(st, on, l, ride);
    if (rc) failed_ = (cfg_.fast ? kStageNameFast : kStageName)[st];
    return rc;
}

// fmd_release_outputs: the writers of this slot's output views wait for the consumer that still reads the old contents
int Schedule::wait_consumer(ScheduleBackend& be, int slot, Queue qx, Queue qr) {
    if (!consumer_pending_[slot]) return 0;
    SCHED_TRY(wait(be, qx, slot_event(EV_C, slot)));
    if (qr != qx) SCHED_TRY(wait(be, qr, slot_event(EV_C, slot)));
    consumer_pending_[slot] = false;
    return 0;
}

// The pilot stage of block b as a launch of its own on `on`: its own queue, or the front end's behind a put-off block's front end.
int Schedule::queue_pilot(ScheduleBackend& be, Block& b, Queue on, bool chained) {
    const bool pipe = cfg_.pipelined, fast = cfg_.fast;
    b.pll_pending = false;
    // consecutive blocks' pilot stages run in order (a block whose stage is queued at submission sends the put-off one ahead)
    if (pipe && fast && last_p_event_ && last_p_queue_ != on) SCHED_TRY(wait(be, on, last_p_event_));
    if (pipe && (on != Q_F || b.front_cross)) SCHED_TRY(wait(be, on, b.front_dep));
    // Tolerance mode: the pilot stage of block k also writes the history in front of the NEXT slot's rows (fm_out tail, last span's cubic),
    // which the extract stage of the block that last used that slot (k - 5) reads.  On the front end's queue that stage sits ahead;
    // otherwise (fmd_process_*, small batches, a consumer holding outputs back) nothing else orders the two.
    if (pipe && fast && on != Q_F) {
        const int nx = (b.slot + 1) % kSlots;
        if (slot_used_[nx] && x_done_[nx]) SCHED_TRY(wait(be, on, x_done_[nx]));
    }
    SCHED_TRY(run(be, ST_PLL, on, b, slot_event(EV_B, b.slot), &b.pll_dep, chained ? ++pll_seq_ : 0u));
    b.pll_queue = on;
    if (pipe && fast) { last_p_queue_ = on; last_p_event_ = b.pll_dep; }
    return 0;
}

// The extract and RDS stages of block b: extract on qx, RDS on qr; a pilot stage that is still pending goes ahead on q_pilot.
int Schedule::queue_outputs(ScheduleBackend& be, Block& b, Queue qx, Queue qr, Queue q_pilot) {
    const bool pipe = cfg_.pipelined;
    SCHED_TRY(wait_consumer(be, b.slot, qx, qr));
    if (pipe && last_x_event_ && last_x_queue_ != qx) SCHED_TRY(wait(be, qx, last_x_event_));
    if (b.pll_pending) SCHED_TRY(queue_pilot(be, b, q_pilot, false));
    if (pipe && b.pll_dep && b.pll_queue != qx) SCHED_TRY(wait(be, qx, b.pll_dep));
    Event dep;
    // the extract stage's event fires behind k_extract itself: k_rds_sync does not need k_lmr_phase (same queue, behind it)
    SCHED_TRY(run(be, ST_EXTRACT, qx, b, slot_event(EV_E, b.slot), &dep));
    if (pipe) { last_x_queue_ = qx; last_x_event_ = dep; x_done_[b.slot] = dep; }
    if (pipe) SCHED_TRY(wait(be, qr, dep));
    SCHED_TRY(run(be, ST_RDS, qr, b, slot_event(EV_X, b.slot), &dep));
    // X outlives the call (slot reuse, fmd_wait_outputs): when the dispatch carried a timing event instead, record it
    if (pipe && dep != slot_event(EV_X, b.slot)) SCHED_TRY(record(be, slot_event(EV_X, b.slot), qr));
    out_slot_ = b.slot; have_out_ = true; out_block_ = b.block;
    return 0;
}

// behind_front: k_extract_bp goes on the FRONT END's queue.  The two throughput kernels gain nothing from running side by side — together they
// took longer than one after the other (0.37 ms a block for the pair against 0.14 + 0.17 ms alone; they share a CU's LDS and wave slots, and every
// hop between queues costs ~50 us) — so they take turns on one queue, in the order front(k + 1), extract(k), front(k + 2), ...; by the time
// extract(k) is reached, the pilot loop of block k has run, as the RDS stages do on their own queue.  Otherwise (somebody asks for the block's outputs
// before the next block is there) it goes on the extract queue as in the exact mode, beside the next front end.
int Schedule::flush(bool behind_front, ScheduleBackend& be) {
    if (!deferred_.active) return 0;
    deferred_.active = false;
    return queue_outputs(be, deferred_, behind_front ? Q_F : Q_X, Q_R, behind_front ? Q_F : Q_B);
}

// Default: the newest outputs are the newest BLOCK's — if its extract stage is still put off it is queued now, on the extract queue, and from here on
// every block's stages are queued at once (such a caller asks after every block: taking turns on the front end's queue would stall that queue for
// the length of the pilot loop each time).  fmd_set_output_lag: nothing is forced, the views are the newest queued ones.
int Schedule::outputs_wanted(ScheduleBackend& be) {
    if (lag_outputs_ || !deferred_.active) return 0;
    lazy_extract_ = false;
    return flush(false, be);
}

int Schedule::wait_outputs(ScheduleBackend& be) {
    if (!cfg_.pipelined || n_blocks_ == 0) return 0;      // unpipelined: the outputs are already ordered on the caller's stream
    SCHED_TRY(outputs_wanted(be));
    if (!have_out_) return 0;                             // (fmd_set_output_lag before the second block: nothing queued yet)
    return wait(be, Q_CALLER, slot_event(EV_X, out_slot_));
}

int Schedule::release_outputs(ScheduleBackend& be) {
    if (n_blocks_ == 0) return 0;
    SCHED_TRY(outputs_wanted(be));
    if (!have_out_) return 0;
    SCHED_TRY(record(be, slot_event(EV_C, out_slot_), Q_CALLER));
    consumer_pending_[out_slot_] = true;
    return 0;
}

int Schedule::wait_input(ScheduleBackend& be) {
    if (!cfg_.pipelined || n_blocks_ == 0 || !ev_consumed_) return 0;   // unpipelined: the read is already ordered on the submitting stream
    return wait(be, Q_CALLER, ev_consumed_);
}

void Schedule::drained() {
    last_x_event_ = Event{};          // (everything has run: no order left to keep; a timed block's events are about to be freed)
    last_p_event_ = Event{};
    for (Event& e : x_done_) e = Event{};
}

void Schedule::reset() {
    pll_seq_ = 0;
    n_blocks_ = 0;
    warm_left_ = cfg_.fast ? (8192 + cfg_.n_fm_out - 1) / cfg_.n_fm_out : 0;      // kPllWarmSamples of every station's life
    if (cfg_.fast && cfg_.warm_forever) warm_left_ = 1 << 30;                     // k_pll_span for every block
    deferred_.active = false;
    drained();
    ev_consumed_ = Event{};
    out_slot_ = 0; sub_slot_ = 0; have_out_ = false; out_block_ = -1;
    for (bool& u : slot_used_) u = false;
    for (bool& u : consumer_pending_) u = false;
}

int Schedule::submit(const BlockFacts& f, ScheduleBackend& be) {
    const bool pipe = cfg_.pipelined, fast = cfg_.fast;
    const bool ordered = f.ordered || !pipe;       // unpipelined: every stage runs on the caller's stream itself
    const int slot = (int)(n_blocks_ % kSlots), m = cfg_.m;
    Block cur;
    cur.slot = slot; cur.par = (int)(n_blocks_ & 1); cur.block = n_blocks_;
    cur.warm = (fast && warm_left_ > 0) ? (warm_left_ >= (1 << 29) ? 2 : 1) : 0;
    cur.prof_block = f.prof_block; cur.prof_mode = profiling_;
    const Queue sF = pipe ? Q_F : Q_CALLER, sA = pipe ? Q_A : Q_CALLER, sX = pipe ? Q_X : Q_CALLER, sR = pipe ? Q_R : Q_CALLER;
    const bool lazy = pipe && lazy_extract_ && !ordered;
    // consecutive blocks' PLL launches alternate between two queues when they hand over per wavefront (fmd_kernels.hip)
    const bool chained = pipe && plan_->pll_chained;
    const Queue sB = pipe ? ((chained && (n_blocks_ & 1)) ? Q_OWN : Q_B) : Q_CALLER;
    // (here and not with the stages themselves: the RDS stage of a put-off block, queued further down, comes behind this wait too)
    if (!lazy) SCHED_TRY(wait_consumer(be, slot, sX, sR));
    // The first decimator (1.024 / 2.048 MSa/s) gets a queue of its own when the PLL launches do not need the own stream: it then
    // works on block b+1 while k_front works on block b (back to back on one queue the two were the longest stage)
    PlanFacts facts;
    facts.any_deemph = f.any_deemph; facts.deemph_in_tile = f.deemph_in_tile; facts.split_front = f.split_front;
    const bool predecim = m > 1 && !front_takes_capture(*plan_, facts);   // (or one kernel, k_front_pre_mfma)
    const Queue sP = (pipe && m > 1 && !chained) ? Q_OWN : sF;
    // Put-off schedule at 1.024 / 2.048 MSa/s: the front end (with the previous block's pilot stage riding it) follows the first
    // decimator on that queue, and the extract stages have the front end's queue to themselves: two queues that each run ahead,
    // instead of one on which k_extract_bp and the front end take turns while the decimator works beside both.
    const Queue sFq = (lazy && m > 1 && sP != sF && fast) ? sP : sF;
    if (pipe) {
        // input is ready once everything queued so far on the caller's stream has run
        if (ordered || f.have_stream) {
            SCHED_TRY(record(be, slot_event(EV_IN, 0), Q_CALLER));
            SCHED_TRY(wait(be, predecim ? sP : sFq, slot_event(EV_IN, 0)));
        }
        // WAR: this slot's fm_in / fm_out_iq / pilot / pll_dt were last read by the stages of the block kSlots blocks ago
        if (slot_used_[slot]) {
            SCHED_TRY(wait(be, sF, slot_event(EV_X, slot)));
            if (sP != sF) SCHED_TRY(wait(be, sP, slot_event(EV_X, slot)));
        }
    }
    // the block after the last de-emphasised one: k_front maintains the Hilbert history (fo_tail) again and must not overwrite
    // what the previous block's k_hilbert, on its own queue, is still reading
    if (pipe && !f.any_deemph && last_block_deemph_) SCHED_TRY(wait(be, sFq, slot_event(EV_F, sub_slot_)));
    Event input_done;                              // fires when the caller's buffer has been consumed
    if (predecim) {
        SCHED_TRY(run(be, ST_PREDECIM, sP, cur, slot_event(EV_P, slot), &input_done));
        if (pipe && sP != sFq) SCHED_TRY(wait(be, sFq, input_done));
    }
    Event dep;
    {
        // the previous block's pilot stage, put off with its extract stage: as the first workgroups of this launch
        Block& q = deferred_;
        const bool ride = lazy && q.active && q.pll_pending && !q.warm && !q.deemph && q.front_queue == sFq && !f.any_deemph && !cfg_.iq_streams &&
                          !(cfg_.debug_skip & ((1u << ST_PLL) | (1u << ST_FRONT)));
        Launch rider;
        rider.buf = q.slot; rider.par = q.par; rider.warm = q.warm;
        if (ride && last_p_event_ && last_p_queue_ != sFq) SCHED_TRY(wait(be, sFq, last_p_event_));
        SCHED_TRY(run(be, ST_FRONT, sFq, cur, slot_event(f.any_deemph ? EV_D : EV_F, slot), &dep, 0, ride ? &rider : nullptr));
        if (ride) {
            q.pll_pending = false; q.pll_dep = (sFq != sF) ? dep : Event{}; q.pll_queue = sFq;
            last_p_queue_ = sFq; last_p_event_ = dep;          // (the launch's own event)
        }
    }
    const Event front_dep = dep;                   // k_front itself: the caller's buffer (256 kSa/s captures) has been consumed
    if (f.any_deemph) {
        // the optional de-emphasis IIR + Hilbert FIR: a pipeline stage of its own (queue D), so that k_front of the next block
        // runs beside it — in k_front's queue the two made the front end the longest stage (+25 % on the step)
        const Queue sD = pipe ? Q_D : Q_CALLER;
        if (pipe) SCHED_TRY(wait(be, sD, dep));
        SCHED_TRY(run(be, ST_DEEMPH, sD, cur, slot_event(EV_F, slot), &dep));
    }
    if (pipe) {
        const Event consumed = input_done ? input_done : front_dep;
        if (ordered) SCHED_TRY(wait(be, Q_CALLER, consumed));      // the caller may reuse `iq` in stream order after this call
        // fmd_wait_input: an event that outlives this call (a timed stage's stop event belongs to the profiling marks)
        const Event persistent = slot_event(predecim ? EV_P : (f.any_deemph ? EV_D : EV_F), slot);
        if (consumed != persistent) SCHED_TRY(record(be, persistent, predecim ? sP : sFq));
        ev_consumed_ = persistent;
    }
    // (no ordering against the PLL launches: both words only grow, whichever values the copy finds will do)
    if (plan_->pll_k_adaptive && (n_blocks_ & 1) == 0) {
        const int rc = be.copy_pll_hint(sA);
        if (rc) { failed_ = "hipMemcpyAsync"; return rc; }
    }
    if (!fast) {   // (FMD_FLAG_FAST_MATH: the pilot peak filter runs inside the PLL kernel, there is no power pass)
        if (pipe) SCHED_TRY(wait(be, sA, dep));
        SCHED_TRY(run(be, ST_POWER, sA, cur, slot_event(EV_A, slot), &dep));
    }
    cur.front_dep = dep; cur.front_cross = f.any_deemph || sFq != sF; cur.deemph = f.any_deemph; cur.front_queue = sFq; cur.pll_pending = true;
    if (!lazy) {
        if (deferred_.active && deferred_.pll_pending) SCHED_TRY(queue_pilot(be, deferred_, sB, false));     // (the put-off block's pilot stage first)
        SCHED_TRY(queue_pilot(be, cur, sB, chained));
    }
    SCHED_TRY(flush(true, be));                    // the previous block's extract + RDS stages, if they were put off: behind this block's front end
    if (lazy) { deferred_ = cur; deferred_.active = true; }
    else SCHED_TRY(queue_outputs(be, cur, sX, sR, sB));
    last_block_deemph_ = f.any_deemph;
    slot_used_[slot] = true;
    sub_slot_ = slot;
    n_blocks_++;
    if (warm_left_ > 0) warm_left_--;
    return 0;
}

}  // namespace fmd
