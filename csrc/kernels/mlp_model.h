// The reference's MNIST MLP (784 -> 100 sigmoid -> 10, worker.py:46-79): its sizes and the flat
// parameter layout, the ONE definition shared by the fused training step (mlp_step.hip), the
// persistent engine (mlp_persistent.hip) and the evaluation kernel (mlp_eval.hip).
//
// Parameter layout (flat f32, 79,510 elements; gradients use the same layout
// so one all-reduce covers everything):
//   [0, 78400)      W1t [100][784]   (W1t[j][i] = TF kernel W1[i][j])
//   [78400, 78500)  b1  [100]
//   [78500, 79500)  W2t [10][100]    (W2t[c][j] = TF kernel W2[j][c])
//   [79500, 79510)  b2  [10]
#pragma once

namespace dtfx {
namespace mlp_model {

constexpr int D = 784, H = 100, C = 10;
constexpr int HT = 7;          // hidden tiles of 16 (112 padded)
constexpr int HP = HT * 16;    // padded hidden width
constexpr int OFF_W1 = 0;
constexpr int OFF_B1 = H * D;
constexpr int OFF_W2 = OFF_B1 + H;
constexpr int OFF_B2 = OFF_W2 + C * H;
constexpr int NPARAM = OFF_B2 + C;
constexpr int MAXB = 256;      // largest batch of the fused step (mlp_persistent.hip: its own, 128)

static_assert(NPARAM == 79510, "parameter count of worker.py:50-53");

}  // namespace mlp_model
}  // namespace dtfx
