// The central value critic's loss of one row: device code shared by value_loss_kernel (csrc/ppo_loss.hip, see there for
// what it replaces) and the value tail behind a recurrent critic (csrc/rnn_value_tail.hip).
#pragma once

#include "rlg_device.hpp"

namespace rlg {

struct ValueLossRow {
  float c_loss;     // the row's critic loss, before mask and mean
  float d_value;    // d mean(c_loss * mask) / d value
};

// common_losses.critic_loss (clipped or plain, rl_games/common/common_losses.py:16-29) and its gradient for one row:
// torch.max's tie rule (equal branches split the gradient 1/2 + 1/2), clamp's inclusive pass-through range and its NaN
// propagation.  m: the row's mask (1 without masks); denom: fmaxf(sum(mask), 1) or the number of rows.
__device__ __forceinline__ ValueLossRow value_loss_row(float v, float vo, float R, float m, float denom, float e_clip,
                                                       int clip_value) {
  float c_loss, g_v;
  if (clip_value) {
    const float delta = v - vo;
    const float vclip = vo + clamp_nan(delta, -e_clip, e_clip);
    const float d1 = v - R, d2 = vclip - R;
    const float c1 = d1 * d1, c2 = d2 * d2;
    c_loss = fmaxf(c1, c2);
    const float in = (delta >= -e_clip && delta <= e_clip) ? 1.0f : 0.0f;
    if (c1 > c2) g_v = 2.0f * d1; else if (c2 > c1) g_v = 2.0f * d2 * in;
    else g_v = 0.5f * (2.0f * d1) + 0.5f * (2.0f * d2 * in);
  } else {
    const float d = R - v;
    c_loss = d * d;
    g_v = -2.0f * d;
  }
  return ValueLossRow{c_loss, g_v * (m / denom)};
}

}  // namespace rlg
