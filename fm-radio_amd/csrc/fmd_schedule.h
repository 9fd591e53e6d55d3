// The block schedule: which stage of which block goes on which queue, and which events each stage waits for and carries.  Host only (no HIP
// include: tests/cpp/schedule_main.cpp builds it with plain g++ and prints what it asks for; tests/test_schedule_cpu.py compares the
// dependency graph with the one recorded from the code this unit replaced).  Queues and events are names here; fmd_api.cpp's backend maps them
// to hipStream_t / hipEvent_t and makes the HIP calls.
//
// Stage placement: k_front on F, k_pilot_power on A, k_pilot_pll on B, k_extract (+ k_lmr_phase) on X, k_rds_sync on R.  Blocks rotate through
// kSlots buffer slots and every stage waits only for its producer, so in steady state all stages run concurrently on different blocks.
#pragma once

#include "fmd_plan.h"

namespace fmd {

// Stream buffers are indexed by pipeline slot (= block index % kSlots): the stages of consecutive blocks run concurrently
// on different streams, so a producer of block b+1 must not overwrite what a consumer of block b (or b-1) still reads.
// Six slots: the front end and the power pass of a block must be able to run far enough ahead of the PLL that the next PLL
// launch's inputs are ready before the running one ends (with four, the front end of block b+4 waited for the RDS stage of
// block b and the power pass came in ~90 us before the PLL needed it: no room for the per-wavefront hand-over to overlap).
static constexpr int kSlots = 6;

// (the stages themselves, enum Stage, and their kernels' names: fmd_plan.h)

// Q_CALLER: the stream the caller passed to the entry point; Q_OWN: the handle's own stream (host-pointer entry points, uploads, resets; the second
// pilot queue of the per-wavefront hand-over and the first decimator's queue — one more stream would be the ninth on the device with the caller's
// and would share a hardware queue with another stage; everything else the own stream does is preceded by a full synchronisation)
enum Queue { Q_CALLER = 0, Q_OWN, Q_F, Q_D, Q_A, Q_B, Q_X, Q_R, Q_COUNT };

// EV_IN: the caller's input is ready; P F D A B E X: behind the slot's first decimator, front end (fm_out complete), front end while a de-emphasis stage
// follows, power pass, pilot stage, extract stage, RDS stage; C: fmd_release_outputs, the consumer of the slot's outputs has finished with them;
// T0 / T1: start and stop of `stage` in the `slot`-th profiled block (they receive the timestamps of the stage's first and last dispatch packets)
enum EventKind : unsigned char { EV_NONE = 0, EV_IN, EV_P, EV_F, EV_D, EV_A, EV_B, EV_E, EV_X, EV_C, EV_T0, EV_T1 };
struct Event {
    EventKind kind = EV_NONE;
    unsigned char stage = 0;
    int slot = 0;
    explicit operator bool() const { return kind != EV_NONE; }
    bool operator==(const Event& o) const { return kind == o.kind && stage == o.stage && slot == o.slot; }
    bool operator!=(const Event& o) const { return !(*this == o); }
};

// One stage's launch: buf = block % kSlots (stream buffers), par = block & 1 (history tails); seq: 1-based number of the block when consecutive
// blocks' k_pilot_pll launches hand over per wavefront, 0: plain stream order; warm: tolerance mode, a block inside some station's start-up transient
// (2: FMD_DEBUG_PLL_DENSE); t0 / t1: timing events the dispatch packets carry; done: the event that is to fire when the stage's last kernel has
// completed, carried by that kernel's own dispatch packet (a separate record is one more queue packet between two dependent kernels, ~25 us on the
// pilot queue).  A stage that is being timed already carries its stop event there: the next stage then waits on that one.
struct Launch { int buf = 0, par = 0; unsigned seq = 0; int warm = 0; Event t0{}, t1{}, done{}; };

// What the schedule asks of the runtime.  Every call returns 0 or the runtime's error code, which the schedule hands up (Schedule::failed_what()).
struct ScheduleBackend {
    virtual int wait(Queue q, Event e) = 0;
    virtual int record(Event e, Queue q) = 0;
    // ride (front end, tolerance mode only): the pilot stage of that block rides in the same launch
    virtual int launch(Stage st, Queue q, const Launch& l, const Launch* ride) = 0;
    virtual int copy_pll_hint(Queue q) = 0;      // the 8-byte copy of the pilot kernel's out-of-lock counters to the host
    virtual ~ScheduleBackend() = default;
};

// What the schedule needs to know of the handle (fixed at creation, but for the plan, which fmd_debug_pll_adaptive replaces while everything is idle)
struct ScheduleConfig {
    bool fast = false, pipelined = true, iq_streams = false;   // iq_streams: the handle materialises fm_out_iq / pll_dt (Buffers::fm_out_iq[slot] exists)
    int m = 1, n_fm_out = 0;
    bool warm_forever = false;                                 // development knob FMD_DEBUG_PLL_DENSE
    unsigned debug_skip = 0;                                   // development knob FMD_DEBUG_SKIP_STAGES: bit (1 << Stage) = do not launch that stage (timing experiments only: outputs are garbage)
};

// ... and of the block being submitted
struct BlockFacts {
    bool ordered = true;          // fmd_process_*_dev: the caller's stream is ordered behind the library's read of the block; false: fmd_submit_*_dev
    bool have_stream = true;      // fmd_submit_*_dev: a ready stream was passed (NULL = the input is in place now)
    bool any_deemph = false, deemph_in_tile = false, split_front = false;     // LaunchCtx::facts', after the control upload
    int prof_block = -1;          // index of the block's timing events (Schedule::profiling() != 0), or -1
};

class Schedule {
public:
    void init(const ScheduleConfig& c, const Plan* plan) { cfg_ = c; plan_ = plan; lazy_extract_ = plan->lazy_capable; reset(); }

    // Queue one block's stages.  A failure leaves the state between two blocks (the caller poisons the handle).
    int submit(const BlockFacts& f, ScheduleBackend& be);
    // The extract + RDS stages (and the pilot stage, if it has not found a front end to ride) of the block whose launch fmd_submit_* put off:
    // behind_front: on the front end's queue (the next block has just been submitted, or everything drains); otherwise on the extract queue
    int flush(bool behind_front, ScheduleBackend& be);
    // A caller is about to use the device views of the newest outputs
    int outputs_wanted(ScheduleBackend& be);
    int wait_outputs(ScheduleBackend& be);       // fmd_wait_outputs, fmd_release_outputs, fmd_wait_input: the caller's stream is Q_CALLER
    int release_outputs(ScheduleBackend& be);
    int wait_input(ScheduleBackend& be);
    void drained();                              // every queue has been synchronised: no order left to keep
    void reset();                                // the block numbering restarts (callers drain first)
    void set_output_lag(bool on) { lag_outputs_ = on; lazy_extract_ = plan_->lazy_capable; }   // (a caller that asked for every block's outputs at once had switched the put-off schedule off)
    void set_profiling(int mode) { profiling_ = mode; }
    void keep_warm(int blocks) { if (blocks > warm_left_) warm_left_ = blocks; }   // a station restored inside its start-up transient

    int profiling() const { return profiling_; }
    bool outputs_put_off() const { return !lag_outputs_ && deferred_.active; }     // outputs_wanted() would queue stages
    long n_blocks() const { return n_blocks_; }
    int out_slot() const { return out_slot_; }
    bool have_out() const { return have_out_; }
    long out_block() const { return out_block_; }
    unsigned pll_seq() const { return pll_seq_; }
    const char* failed_what() const { return failed_; }      // the stage (by kernel name) or runtime call that returned the last error

private:
    // a block from its front end on: what its remaining stages need
    struct Block {
        bool active = false, pll_pending = false, front_cross = false, deemph = false;
        int slot = 0, par = 0, warm = 0;
        long block = 0;
        int prof_block = -1, prof_mode = 0;      // its timing events and the sampling rule in force when it was submitted
        Queue front_queue = Q_F, pll_queue = Q_B;
        Event front_dep{}, pll_dep{};            // behind front_dep the block's fm_out is complete; pll_dep: behind the pilot stage (none: it rode the front end on the extract stage's queue)
    };
    bool timed(const Block& b, Stage st) const;
    int run(ScheduleBackend& be, Stage st, Queue on, const Block& b, Event done, Event* dep, unsigned seq = 0, const Launch* ride = nullptr);
    int wait(ScheduleBackend& be, Queue q, Event e);
    int record(ScheduleBackend& be, Event e, Queue q);
    int wait_consumer(ScheduleBackend& be, int slot, Queue qx, Queue qr);
    int queue_pilot(ScheduleBackend& be, Block& b, Queue on, bool chained);
    int queue_outputs(ScheduleBackend& be, Block& b, Queue qx, Queue qr, Queue q_pilot);

    ScheduleConfig cfg_{};
    const Plan* plan_ = nullptr;
    const char* failed_ = "";
    // Tolerance mode, fmd_submit_*: k_extract_bp shares k_front_mfma's queue and a block's extract + RDS stages are queued when the NEXT block is
    // submitted (behind that block's front end) or when somebody asks for the outputs.  Its pilot stage has not been queued either: it rides in the
    // next block's front-end launch (k_front_mfma<FUSED>) or, where that is not possible (a start-up block, the getters' per-sample streams, a flush),
    // goes in front of the extract stage on its own.
    bool lazy_extract_ = false, lag_outputs_ = false;
    Block deferred_{};
    Queue last_x_queue_ = Q_X, last_p_queue_ = Q_B;
    Event last_x_event_{};                // behind the newest extract stage: consecutive blocks' extract stages are ordered (L-R phase estimate), whichever of the two queues they take
    Event last_p_event_{};                // behind the newest pilot stage (tolerance mode): consecutive blocks' pilot stages run in order (loop state), whichever queue each takes; none: drained
    Event x_done_[kSlots] = {};           // fires when the extract stage of the block in that slot has run; none: drained
    bool slot_used_[kSlots] = {};
    bool consumer_pending_[kSlots] = {};  // fmd_release_outputs: a consumer still reads the slot's old outputs
    bool last_block_deemph_ = false;      // the previous block went through the de-emphasis stage (queue D)
    unsigned pll_seq_ = 0;                // k_pilot_pll launches handed over per wavefront so far (0: hand-over by stream order)
    int warm_left_ = 0;                   // tolerance mode: blocks still inside some station's start-up transient (k_pll_span runs beside k_pll_sparse)
    long n_blocks_ = 0;                   // blocks submitted since create / reset; slot = n_blocks % kSlots
    int out_slot_ = 0;                    // slot holding the newest outputs (the newest block's; under fmd_set_output_lag: the newest QUEUED outputs)
    int sub_slot_ = 0;                    // slot of the newest submitted block
    bool have_out_ = false;               // some block's output stages have been queued since create / reset
    long out_block_ = -1;                 // ... and which block's (0 = the first since create / reset) the output views are
    Event ev_consumed_{};                 // fires when the newest block's input buffer has been read (fmd_wait_input)
    int profiling_ = 0;                   // 0 off, 1 every kernel of every block, 2 k_pilot_pll every block + the rest every 4th, 3 every stage of every 4th block + the pilot stage behind it
};

}  // namespace fmd
