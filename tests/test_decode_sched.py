"""The decode loop's poll schedule (capdec_amd/csrc/decode_sched.h) on the host: no GPU needed.

A small stand-alone C++ program around the header runs the step loop of the decode drivers with the device taken out: it
reads, per case, the caption count, the first step, T, the activation rows per caption, the compaction switch and the alive
count a poll in front of each step would find, and prints per step whether it polled, whether it compacted and the rows it
launched.  ``loop_model`` below is the same loop in Python, written from decode_chunk's loop as it stood before the header
existed (poll when due, stop at zero alive, row tiers 8192 / 2048 / 512 -> base interval 1 / 2 / 4 / 8, a poll that finds
nothing finished doubles the interval up to 8, compaction once at least max(1, na / 32) captions are gone); the two must
agree step for step.  tests/test_decode_loop.py imports the model and holds every driver's statistics against it on the
GPU."""
import os
import random
import subprocess
from typing import NamedTuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "capdec_amd", "csrc")


class Loop(NamedTuple):
    polled: list          # per step run: a poll in front of it
    compacted: list       # ... a compaction in front of it
    rows: list            # ... activation rows launched (decode_step_rows)
    steps: int            # decode_stats: steps, the prefill's selection counted (first_step 1) or not (first_step 0)
    compactions: int
    row_steps: int
    polled_zero: bool     # the loop ended at a poll that found nobody alive


def loop_model(nc, first_step, T, rows_per_caption, compact, alive):
    """alive[i - first_step]: captions still generating at a poll in front of step i (read only where a poll happens)"""
    na, next_poll, backoff, last_alive = nc, 1, 1, nc + 1
    polled, compacted, rows = [], [], []
    steps = 1 if first_step == 1 and nc > 0 else 0
    zero = False
    for i in range(first_step, T):
        p = c = False
        if i >= next_poll:
            a = alive[i - first_step]
            if a == 0:
                zero = True
                break
            p = True
            rows_now = a * rows_per_caption
            base = 1 if rows_now >= 8192 else 2 if rows_now >= 2048 else 4 if rows_now >= 512 else 8
            backoff = 1 if a < last_alive else min(8, backoff * 2)
            last_alive = a
            next_poll = i + min(8, max(base, backoff))
            if compact and a <= na - max(1, na // 32):
                na, c = a, True
        steps = max(steps, i + 1)
        polled.append(p)
        compacted.append(c)
        rows.append(na * rows_per_caption)
    return Loop(polled, compacted, rows, steps, sum(compacted), sum(rows), zero)


def alive_from_lengths(lens, first_step, T):
    """the alive counts a call's returned lengths imply: a caption whose longest beam has length L is still generating at the
    poll in front of step i exactly when L > i (token i - 1 was not its stop token)"""
    return [sum(1 for L in lens if L > i) for i in range(first_step, T)]


MAIN = r"""
#include <cstdio>
#include <vector>
#include "decode_sched.h"
using namespace capdec;
int main() {
    int nc, first, T, rpc, compact;
    while (scanf("%d %d %d %d %d", &nc, &first, &T, &rpc, &compact) == 5) {
        std::vector<int> alive(T > first ? T - first : 0);
        for (int &a : alive)
            if (scanf("%d", &a) != 1) return 1;
        PollSchedule sched(nc);
        int na = nc;
        for (int i = first; i < T; ++i) {
            int polled = 0, compacted = 0;
            if (sched.due(i)) {
                const int a = alive[i - first];
                if (a == 0) break;
                polled = 1;
                sched.polled(i, a, rpc);
                if (compact && compaction_pays(na, a)) { na = a; compacted = 1; }
            }
            printf("%d %d %d\n", polled, compacted, na * rpc);
        }
        printf("end\n");
    }
    return 0;
}
"""


def build_sched(tmp, flags=()):
    src = os.path.join(tmp, "decode_sched_main.cpp")
    with open(src, "w") as f:
        f.write(MAIN)
    exe = os.path.join(tmp, "decode_sched_main" + ("_san" if flags else ""))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", *flags, "-I", CSRC, src, "-o", exe], check=True)
    return exe


def run_sched(exe, cases):
    """cases: (nc, first_step, T, rows_per_caption, compact, alive) -> per case the (polled, compacted, rows) lists"""
    text = "".join(" ".join(str(int(v)) for v in (*c[:5], *c[5])) + "\n" for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("end\n")
    assert len(out) == len(cases) + 1 and out[-1] == ""
    res = []
    for block in out[:-1]:
        v = [[int(x) for x in line.split()] for line in block.splitlines()]
        res.append(([bool(r[0]) for r in v], [bool(r[1]) for r in v], [r[2] for r in v]))
    return res


def falling(nc, first, T, keep):
    """alive counts that fall geometrically: keep ** k of nc at the k-th step"""
    return [int(nc * keep ** (k + 1)) for k in range(T - first)]


def cases():
    rnd = random.Random(5)
    out = {
        # 10 000 rows down to 95: >= 8192, >= 2048, >= 512 and below
        "four_tiers": (2000, 1, 60, 5, 1, [max(19, int(2000 * 0.93 ** k)) for k in range(1, 60)]),
        "nothing_finishes": (100, 1, 67, 5, 1, [100] * 66),
        "nothing_finishes_large": (2000, 1, 67, 5, 1, [2000] * 66),
        "all_done_at_step_1": (64, 1, 12, 5, 1, [0] * 11),
        # one caption of 640 per step: below na / 32 = 20 at every poll until the losses add up
        "slow_loss": (640, 1, 67, 5, 1, [640 - k for k in range(1, 67)]),
        "first_step_0": (300, 0, 30, 4, 1, [300] + falling(300, 1, 30, 0.85)),
        "first_step_0_done_at_1": (16, 0, 12, 4, 1, [16] + [0] * 11),
        # 900 captions x 10 rows: the 9000 rows poll every step, 4500 would poll every other
        "ten_rows_per_caption": (900, 1, 20, 10, 1, [900 - 3 * k for k in range(1, 20)]),
        "compaction_off": (2000, 1, 40, 5, 0, falling(2000, 1, 40, 0.8)),
        "T_1": (16, 1, 1, 5, 1, []),
    }
    for k in range(300):
        nc, first, T = rnd.choice((1, 7, 16, 100, 625, 1700, 5000)), rnd.choice((0, 1)), rnd.randint(1, 70)
        a, seq = nc, []
        for _ in range(T - first):
            if rnd.random() < 0.5:
                a -= rnd.randint(0, max(1, a // rnd.choice((2, 8, 40, 200))))
            seq.append(max(a, 0))
        out[f"random_{k}"] = (nc, first, T, rnd.choice((1, 2, 4, 5, 8, 10)), rnd.random() < 0.8, seq)
    return out


def check_against_model(exe):
    cs = cases()
    got = run_sched(exe, list(cs.values()))
    for (name, c), (polled, compacted, rows) in zip(cs.items(), got):
        want = loop_model(*c)
        assert (polled, compacted, rows) == (want.polled, want.compacted, want.rows), (name, c[:5])
    return cs


def test_schedule_against_the_model(tmp_path):
    cs = check_against_model(build_sched(str(tmp_path)))
    m = {k: loop_model(*c) for k, c in cs.items()}
    # the cases walk what they are there for
    t = m["four_tiers"]

    def gaps(l):
        at = [i for i, p in enumerate(l.polled) if p]
        return [b - a for a, b in zip(at, at[1:])]
    assert t.rows[0] >= 8192 and t.rows[-1] < 512 and {1, 2, 4, 8} <= set(gaps(t)), (t.rows, gaps(t))
    for name in ("nothing_finishes", "nothing_finishes_large"):
        n = m[name]
        at = [i for i, p in enumerate(n.polled) if p]
        # the first poll (step 1) keeps the base interval, then every poll doubles it up to 8; no compaction, no row less
        base = 8 if name == "nothing_finishes" else 1
        assert at[0] == 0 and gaps(n)[:4] == [max(base, 1), max(base, 2), max(base, 4), 8] and set(gaps(n)[3:]) == {8}, gaps(n)
        assert n.compactions == 0 and len(set(n.rows)) == 1 and n.steps == 67
    d = m["all_done_at_step_1"]
    assert d.rows == [] and d.steps == 1 and d.polled_zero
    s = m["slow_loss"]
    assert s.compactions >= 1 and not s.compacted[0] and s.polled[0] and s.rows[0] == 640 * 5
    assert all(640 * 5 - r >= 20 * 5 for r in s.rows if r != 640 * 5)
    z = m["first_step_0"]
    assert not z.polled[0] and z.polled[1] and z.rows[0] == 1200 and z.steps == 30 and len(z.rows) == 30
    z1 = m["first_step_0_done_at_1"]
    assert z1.rows == [64] and z1.steps == 1 and z1.polled_zero
    r = m["ten_rows_per_caption"]
    assert all(r.polled[:4]) and r.rows[0] == 9000
    assert m["compaction_off"].compactions == 0 and m["T_1"].rows == [] and m["T_1"].steps == 1


def test_schedule_under_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone host program, nothing preloaded"""
    check_against_model(build_sched(str(tmp_path), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


def test_alive_from_lengths():
    assert alive_from_lengths([1, 3, 12, 12], 1, 12) == [3, 3, 2] + [2] * 8
    assert alive_from_lengths([1, 3, 12], 0, 12) == [3, 2, 2] + [1] * 9
