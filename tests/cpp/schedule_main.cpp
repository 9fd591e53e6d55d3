// fm-radio_amd/csrc/fmd_schedule.cpp with fmd_plan.cpp on their own (no HIP, no library): the block schedule driven by a backend that prints.
// `make -C oracle asan` builds it with -fsanitize=address,undefined; tests/test_schedule_cpu.py builds it plain.
//
// Reads scenarios:   scenario NAME stations block_size fs_baseband flags
//                    one call a line (below)
//                    end
// and writes "== NAME", then one line per backend call (wait Q EV | record EV Q | launch STAGE Q buf= par= seq= warm= t0= t1= done= ride= | copy_hint Q),
// each call echoed behind "# " in front of its lines, then "== end".  Around the schedule it does what fmd_api.cpp does around it: the facts of a block
// (de-emphasis on, in k_front's tile or as a stage, lingering one block), the drain in front of a control upload and of the hooks, the timing events'
// block index.
#include <cstdio>
#include <cstring>
#include <string>

#include "fmd_schedule.h"

using namespace fmd;

namespace {

const char* const kQueue[Q_COUNT] = {"caller", "own", "F", "D", "A", "B", "X", "R"};
const char* const kStage[ST_COUNT] = {"front", "deemph", "power", "pll", "extract", "rds", "predecim"};

std::string name(Event e) {
    switch (e.kind) {
        case EV_NONE: return "-";
        case EV_IN: return "in";
        case EV_T0: case EV_T1: return std::string(e.kind == EV_T0 ? "t0:" : "t1:") + kStage[e.stage] + ":" + std::to_string(e.slot);
        default: return std::string(1, "??PFDABEXC"[e.kind]) + std::to_string(e.slot);
    }
}

struct Printer : ScheduleBackend {
    int wait(Queue q, Event e) override { std::printf("wait %s %s\n", kQueue[q], name(e).c_str()); return 0; }
    int record(Event e, Queue q) override { std::printf("record %s %s\n", name(e).c_str(), kQueue[q]); return 0; }
    int launch(Stage st, Queue q, const Launch& l, const Launch* ride) override {
        char rb[64] = "-";
        if (ride) std::snprintf(rb, sizeof(rb), "%d,%d,%u,%d", ride->buf, ride->par, ride->seq, ride->warm);
        std::printf("launch %s %s buf=%d par=%d seq=%u warm=%d t0=%s t1=%s done=%s ride=%s\n", kStage[st], kQueue[q], l.buf, l.par, l.seq, l.warm, name(l.t0).c_str(),
                    name(l.t1).c_str(), name(l.done).c_str(), rb);
        return 0;
    }
    int copy_pll_hint(Queue q) override { std::printf("copy_hint %s\n", kQueue[q]); return 0; }
};

// one handle, as far as the schedule can tell
struct Handle {
    int C = 0, m = 1, n_fm_out = 0, n_est = 0;
    unsigned flags = 0;
    bool fast = false;
    Plan plan{};
    Schedule sched;
    Printer out;
    // fmd_api.cpp upload_controls(): 0 no station filters, 1 every time constant fits k_front's tile (50 us), 2 one does not (150 us)
    int controls = 0;
    bool controls_dirty = true, deemph_on = false, deemph_linger = false, any_deemph = false, deemph_in_tile = false, split_front = false;
    int n_profiled = 0;

    void create(int stations, int block, int fs, unsigned fl) {
        C = stations; flags = fl; m = fs / 256000; fast = (fl & FMD_FLAG_FAST_MATH) != 0;
        n_fm_out = block / m / 2;
        const int n_audio = n_fm_out / 4;
        n_est = (n_audio + 9) / 10;
        plan = make_plan(C, m, n_fm_out, n_est, flags);
        ScheduleConfig c;
        c.fast = fast; c.pipelined = (fl & FMD_FLAG_NO_PIPELINE) == 0; c.m = m; c.n_fm_out = n_fm_out;
        c.iq_streams = !fast || (fl & FMD_FLAG_KEEP_TAPS) || (n_audio % 256) != 0;
        sched.init(c, &plan);
    }
    int sync() { const int rc = sched.flush(true, out); sched.drained(); return rc; }
    void upload_controls() {
        const bool any = controls != 0;
        deemph_in_tile = fast && controls == 1;
        if (deemph_in_tile) { any_deemph = false; deemph_linger = false; deemph_on = false; }
        else {
            if (any) { any_deemph = true; deemph_linger = false; }
            else if (deemph_on) { any_deemph = true; deemph_linger = true; }
            else if (!deemph_linger) any_deemph = false;
            deemph_on = any;
        }
        controls_dirty = false;
    }
    int block(bool ordered, bool have_stream) {
        if (controls_dirty) { if (int rc = sync()) return rc; upload_controls(); }
        BlockFacts f;
        f.ordered = ordered; f.have_stream = have_stream;
        f.any_deemph = any_deemph; f.deemph_in_tile = deemph_in_tile; f.split_front = split_front;
        f.prof_block = sched.profiling() ? n_profiled++ : -1;
        const int rc = sched.submit(f, out);
        if (deemph_linger) { deemph_linger = false; any_deemph = false; }
        return rc;
    }
    int call(const char* op, int a, int b) {
        if (!std::strcmp(op, "process")) return block(true, true);
        if (!std::strcmp(op, "submit")) return block(false, a != 0);
        if (!std::strcmp(op, "wait_outputs")) return sched.wait_outputs(out);
        if (!std::strcmp(op, "release_outputs")) return sched.release_outputs(out);
        if (!std::strcmp(op, "wait_input")) return sched.wait_input(out);
        if (!std::strcmp(op, "synchronize")) return sync();
        if (!std::strcmp(op, "reset")) {
            const int rc = sync();
            sched.reset();
            deemph_on = false; deemph_linger = false; any_deemph = false; controls_dirty = true;
            return rc;
        }
        if (!std::strcmp(op, "set_output_lag")) { const int rc = sync(); sched.set_output_lag(a != 0); return rc; }
        if (!std::strcmp(op, "controls")) { controls = a; controls_dirty = true; return 0; }
        if (!std::strcmp(op, "profile")) { sched.set_profiling(a); return 0; }
        if (!std::strcmp(op, "pll_adaptive")) {
            const int rc = sync();
            const PllThresholds moved{a, b};
            plan = make_plan(C, m, n_fm_out, n_est, flags, &moved);
            return rc;
        }
        if (!std::strcmp(op, "split_front")) { const int rc = sync(); split_front = a != 0; return rc; }
        return -1;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: schedule_main scenarios.txt\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    char line[256], op[64], nm[128];
    Handle* h = nullptr;
    int n = 0, bad = 0;
    while (std::fgets(line, sizeof(line), f)) {
        int a = 0, b = 0;
        if (std::sscanf(line, "%63s", op) != 1) continue;
        if (!std::strcmp(op, "scenario")) {
            int stations, block, fs;
            unsigned flags;
            if (h || std::sscanf(line, "%*s %127s %d %d %d %u", nm, &stations, &block, &fs, &flags) != 5 || stations <= 0 || fs < 256000 || block < 2048 * (fs / 256000)) { bad = 1; break; }
            h = new Handle();
            h->create(stations, block, fs, flags);
            std::printf("== %s\n", nm);
            n++;
        } else if (!std::strcmp(op, "end")) {
            if (!h) { bad = 1; break; }
            std::printf("== end\n");
            delete h;
            h = nullptr;
        } else {
            if (!h) { bad = 1; break; }
            std::sscanf(line, "%*s %d %d", &a, &b);
            std::printf("# %s", line);
            if (h->call(op, a, b)) { bad = 1; break; }
        }
    }
    delete h;
    std::fclose(f);
    if (bad) std::fprintf(stderr, "schedule_main: bad line: %s", line);
    return (bad || n == 0) ? 1 : 0;
}
