// rx_track_duel.h -- the rules of the TRACK CURRICULUM FOR SELF-PLAY (rx_track_tally2 /
// rx_track_duel_scores / rx_track_duel_rollout_steps, ABI v25 additive) as inline
// functions compiled twice, beside rx_curriculum.h and under its discipline: hipcc for
// gfx950 (rx_curriculum.hip) and plain C++ for the host twins (rx_curriculum_host.cpp);
// float64 with every operation separately rounded, integer weights and integer sums, so
// the kernel, the host twin and a Python restatement (tests/test_track_selfplay_cpu.py)
// agree bit for bit.
//
// Rules (DESIGN.md §4 "Track curriculum for self-play"):
//  * a two-car env e that ended (done[e] != 0) on slot k = track[e] inside the table, with
//    a = the learner's car, o = 1 - a, info the terminal step's rows [n][2][RX_INFO_W]:
//      pa = info[e][a][PROGRESS], po = info[e][o][PROGRESS], la = info[e][a][PLACEMENT]
//    tally[k] (the single-agent columns, read for the learner's car):
//      episodes += 1;  finishes += (pa == 1.0);
//      crashes  += (terminated and pa != 1.0 and po != 1.0)   -- BOTH cars left the track,
//                  the only way a two-car episode terminates without a finish; a lost race
//                  is not a crash, which is why rx_tc_outcome is not used here;
//      progress_q += (int64)(pa * 2^20)
//    duel[k]:
//      wins += (la == 1.0);  opp_finishes += (po == 1.0);
//      opp_progress_q += (int64)(po * 2^20);  timeouts += (not terminated)
//    Placement 1 is always awarded when an episode ends, so losses = episodes - wins.
//  * scores: 0 "fail" and 1 "potential" are rx_tc_weight on (episodes, finishes); 2 "lose"
//    and 3 "contested" are the SAME arithmetic on the two-entry row (episodes, wins):
//      p_k = (wins + prior) / (episodes + 2 * prior)
//      q_k = 1 - p_k (lose)   or   4 * p_k * (1 - p_k) (contested)
//    f_k, W_k and the exact integer cdf are rx_tc_weight's, unchanged.
//  * the draw is rx_tc_draw: it reads cdf only.
#pragma once

#include "rx_curriculum.h"

// RX_TRACK_DUEL_W (rx.h): wins, opp_finishes, opp_progress_q, timeouts
#define RX_TRACK_SCORE_LOSE 2
#define RX_TRACK_SCORE_CONTESTED 3

#define RX_TD_FINISHED 1
#define RX_TD_CRASHED 2
#define RX_TD_WON 4
#define RX_TD_OPP_FINISHED 8
#define RX_TD_TIMEOUT 16

// what one ended two-car episode adds, as flags (the progress sums go through rx_tc_progress_q)
RX_FN int rx_td_outcome(double pa, double po, double la, uint8_t terminated) {
  const int fin = pa == 1.0 ? 1 : 0, ofin = po == 1.0 ? 1 : 0;
  return (fin ? RX_TD_FINISHED : 0) | ((terminated != 0 && !fin && !ofin) ? RX_TD_CRASHED : 0) |
         (la == 1.0 ? RX_TD_WON : 0) | (ofin ? RX_TD_OPP_FINISHED : 0) | (terminated == 0 ? RX_TD_TIMEOUT : 0);
}

// W_k of one slot from its tally and duel rows; *p_out = the p_k that was used
RX_FN uint64_t rx_td_weight(const int64_t* t, const int64_t* d, int score, int power, double prior, double* p_out) {
  const int64_t row[2] = {t[0], score >= RX_TRACK_SCORE_LOSE ? d[0] : t[1]};
  return rx_tc_weight(row, score & 1, power, prior, p_out);  // lose -> fail's q, contested -> potential's
}
