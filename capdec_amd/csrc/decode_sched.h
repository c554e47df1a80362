// When the decode loop (decode.hip: decode_steps) polls the alive count and when it compacts the batch: host arithmetic only,
// nothing of HIP, so that a plain C++ compiler can build it (tests/test_decode_sched.py does).
//
// Finished captions (stop token on every beam) are dropped from the batch at the poll points.  Poll cadence: a poll drains the
// stream (a 4-byte copy + a synchronisation: ~150 us of idle GPU by the time the host has woken up and refilled the queue).
// While captions ARE finishing a poll pays for itself -- every step that still carries finished captions costs more: a step
// of >= 8192 rows takes >= 8 ms, one of ~3000 rows ~4 ms (round 6, captions that stop after ~11 tokens: with a poll every 8
// steps 25 000 rows were launched for 8 steps while 40 % of them had finished; 519 k row-steps against 427 k alive) -- so the
// base interval is 1 step at >= 8192 rows, 2 at >= 2048, 4 at >= 512, 8 below.  While NOTHING finishes (the synthetic headline
// weights never emit the stop id) every poll is pure loss: each poll that finds no finished caption doubles the interval (up
// to 8), the first one that does resets it.
#pragma once
#include <algorithm>

namespace capdec {

struct PollSchedule {
    int next_poll = 1, backoff = 1, last_alive;
    explicit PollSchedule(int ncap) : last_alive(ncap + 1) {}      // (+ 1: the first poll never backs off)
    bool due(int step) const { return step >= next_poll; }
    // the poll in front of `step` found `alive` captions still generating; a caption is rows_per_caption activation rows
    void polled(int step, int alive, int rows_per_caption) {
        const int rows_now = alive * rows_per_caption;
        const int base = rows_now >= 8192 ? 1 : rows_now >= 2048 ? 2 : rows_now >= 512 ? 4 : 8;
        backoff = alive < last_alive ? 1 : std::min(8, backoff * 2);
        last_alive = alive;
        next_poll = step + std::min(8, std::max(base, backoff));
    }
};

// a batch of na captions of which `alive` still generate: is rebuilding the compaction map worth its launch?
inline bool compaction_pays(int na, int alive) { return alive <= na - std::max(1, na / 32); }

}  // namespace capdec
