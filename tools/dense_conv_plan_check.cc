// The host plan of the dense Conv1d (wekws_amd/csrc/dense_conv_plan.h) under the host sanitizers: a stand-alone program, no
// device, no Python.  It drives the check, grid and workspace functions over the test matrix's shapes, a sweep of small shapes and
// the limits' edges, and holds what needs no reference: a refused shape has a reason and an accepted one has none; Tout, the rows,
// the grids and the workspace are positive, fit their types and obey the header's arithmetic (K times the Linear weight
// gradient's workspace, a multiple of 16 bytes; the pointwise plan's grids); the call checks refuse what they say they refuse.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I wekws_amd/csrc tools/dense_conv_plan_check.cc -o dcp && ./dcp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "dense_conv_plan.h"

namespace {

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Shape { int64_t B, Ci, Tin, Co, K, d, P; };

int accepted = 0, refused = 0;

void accept(const Shape& s) {
  using namespace wekws;
  CHECK(!dense_conv_shape_check(s.B, s.Ci, s.Tin, s.Co, s.K, s.d, s.P));
  const int64_t Tout = dense_conv_tout(s.Tin, s.K, s.d, s.P), R = dense_conv_rows(s.B, Tout);
  CHECK(Tout >= 1 && Tout <= s.Tin && Tout == s.Tin + s.P - (s.K - 1) * s.d && R == s.B * Tout);
  CHECK(dense_conv_stages(s.Ci, s.K) == s.K * ((s.Ci + kPwStage - 1) / kPwStage));
  CHECK(dense_conv_lds_bytes() == pointwise_conv_lds_bytes() && dense_conv_lds_bytes() <= 64 * 1024);
  const int64_t tap = dense_conv_tap_workspace_bytes(s.B, s.Ci, Tout, s.Co), all = dense_conv_workspace_bytes(s.B, s.Ci, Tout, s.Co, s.K);
  CHECK(tap == linear_wgrad_workspace_bytes(R, s.Co, s.Ci) && tap > 0 && tap % 16 == 0 && all == s.K * tap);
  CHECK(dense_conv_grid(s.B, Tout, s.Co) == pointwise_conv_grid(s.B, Tout, s.Co) && dense_conv_grid(s.B, s.Tin, s.Ci) >= 1);
  const char* grid = dense_conv_grid_check(s.B, s.Ci, s.Tin, s.Co, s.K, s.d, s.P);
  const bool fits = dense_conv_grid(s.B, Tout, s.Co) <= INT32_MAX && dense_conv_grid(s.B, s.Tin, s.Ci) <= INT32_MAX &&
                    linear_wgrad_grid(R, s.Co, s.Ci) <= INT32_MAX && linear_wgrad_fold_grid(s.Co, s.Ci) <= INT32_MAX;
  CHECK((grid == nullptr) == fits);
  // the call checks: operands, wants, workspace
  alignas(16) static char buf[64];
  const void* p = buf;
  const char* f = dense_conv_forward_check(p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, p);
  CHECK((f == nullptr) == fits);
  if (fits) {
    CHECK(dense_conv_forward_check(nullptr, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, p));
    CHECK(dense_conv_forward_check(p, s.B, s.Ci, s.Tin, nullptr, s.Co, s.K, s.d, s.P, p));
    CHECK(dense_conv_forward_check(p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, nullptr));
    const size_t n = size_t(all);
    CHECK(!dense_conv_backward_check(p, p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, p, p, p, p, n));
    CHECK(!dense_conv_backward_check(p, p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, p, nullptr, nullptr, nullptr, 0));   // grad_x alone
    CHECK(dense_conv_backward_check(p, p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, nullptr, nullptr, nullptr, p, n));
    CHECK(dense_conv_backward_check(nullptr, p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, p, p, p, p, n));
    CHECK(dense_conv_backward_check(p, nullptr, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, p, p, p, p, n));
    CHECK(dense_conv_backward_check(p, p, s.B, s.Ci, s.Tin, nullptr, s.Co, s.K, s.d, s.P, p, p, p, p, n));
    CHECK(dense_conv_backward_check(p, p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, p, p, nullptr, nullptr, n));
    CHECK(dense_conv_backward_check(p, p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, nullptr, nullptr, p, buf + 8, n));
    CHECK(dense_conv_backward_check(p, p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, nullptr, p, nullptr, p, n - 1));
    if (s.K > 1) CHECK(dense_conv_backward_check(p, p, s.B, s.Ci, s.Tin, p, s.Co, s.K, s.d, s.P, nullptr, p, p, p, size_t(tap)));
  }
  ++accepted;
}

void refuse(const Shape& s, const char* word) {
  const char* why = wekws::dense_conv_shape_check(s.B, s.Ci, s.Tin, s.Co, s.K, s.d, s.P);
  CHECK(why && std::strstr(why, word));
  alignas(16) static char buf[16];
  const char* f = wekws::dense_conv_forward_check(buf, s.B, s.Ci, s.Tin, buf, s.Co, s.K, s.d, s.P, buf);
  const char* b = wekws::dense_conv_backward_check(buf, buf, s.B, s.Ci, s.Tin, buf, s.Co, s.K, s.d, s.P, buf, buf, buf, buf, size_t(-1));
  CHECK(f && b && !std::strcmp(f, why) && !std::strcmp(b, why));
  ++refused;
}

}  // namespace

int main() {
  const int64_t big = INT32_MAX;
  // the test matrix's shapes (tests/dense_conv_matrix.py) and the recipe's
  const Shape matrix[] = {{2, 16, 1, 16, 3, 2, 4},     {2, 16, 129, 16, 3, 2, 4},  {2, 20, 50, 24, 1, 1, 0},   {2, 16, 40, 16, 2, 3, 3},
                          {2, 16, 40, 16, 3, 3, 0},    {2, 16, 40, 16, 3, 3, 2},   {2, 16, 40, 16, 8, 1, 3},   {2, 8, 100, 8, 8, 8, 56},
                          {2, 20, 50, 24, 3, 1, 0},    {2, 16, 3, 16, 8, 1, 7},    {2, 3, 40, 2, 2, 255, 255}, {2, 2, 20, 3, 32, 8, 248},
                          {2, 1, 35, 65, 3, 2, 4},     {2, 65, 35, 65, 3, 2, 4},   {3, 8, 200, 8, 3, 2, 4},    {5, 4, 103, 4, 3, 1, 2},
                          {5, 1025, 3073, 2, 2, 1, 1}, {256, 64, 100, 64, 8, 1, 7}, {256, 64, 100, 64, 8, 8, 56}, {256, 40, 100, 64, 3, 1, 0}};
  for (const Shape& s : matrix) accept(s);
  // every small (K, d, P, Tin): accepted exactly when the rules say so
  for (int64_t K = 1; K <= 33; ++K)
    for (int64_t d = 0; d <= 9; ++d)
      for (int64_t P = -1; P <= (K - 1) * d + 1; ++P)
        for (int64_t Tin : {int64_t(1), int64_t(2), (K - 1) * d - P, (K - 1) * d - P + 1, int64_t(300)}) {
          const bool ok = K <= 32 && d >= 1 && (K - 1) * d + 1 <= 256 && P >= 0 && P <= (K - 1) * d && Tin >= 1 && Tin + P - (K - 1) * d >= 1;
          const Shape s{3, 5, Tin, 7, K, d, P};
          CHECK((wekws::dense_conv_shape_check(s.B, s.Ci, s.Tin, s.Co, s.K, s.d, s.P) == nullptr) == ok);
          if (ok) accept(s);
        }
  // the limits' edges
  accept({1, 1, 1, 1, 1, 1, 0});
  accept({2, 65535, 9, 65535, 3, 1, 2});
  accept({2, 4, 300, 4, 2, 255, 255});
  accept({2, 4, 300, 4, 32, 8, 0});
  accept({1, 4, big, 4, 3, 1, 2});
  accept({big, 4, 1, 4, 2, 1, 1});
  accept({big, 4, 65, 4, 2, 1, 1});                       // accepted as a shape; its grids do not fit one launch
  accept({int64_t(1) << 20, 8, int64_t(1) << 13, 8, 8, 4, 28});
  refuse({0, 4, 9, 4, 3, 1, 2}, "B must");
  refuse({big + 1, 4, 9, 4, 3, 1, 2}, "B must");
  refuse({2, 0, 9, 4, 3, 1, 2}, "Ci must");
  refuse({2, 65536, 9, 4, 3, 1, 2}, "Ci must");
  refuse({2, 4, 0, 4, 3, 1, 2}, "Tin must");
  refuse({2, 4, big + 1, 4, 3, 1, 2}, "Tin must");
  refuse({2, 4, 9, 0, 3, 1, 2}, "Co must");
  refuse({2, 4, 9, 65536, 3, 1, 2}, "Co must");
  refuse({2, 4, 9, 4, 0, 1, 0}, "K must");
  refuse({2, 4, 99, 4, 33, 1, 32}, "K must");
  refuse({2, 4, 9, 4, 3, 0, 0}, "dilation");
  refuse({2, 4, 300, 4, 2, 256, 256}, "window");
  refuse({2, 4, 300, 4, 32, 9, 0}, "window");
  refuse({2, 4, 9, 4, 3, 1, -1}, "left_pad");
  refuse({2, 4, 9, 4, 3, 1, 3}, "left_pad");
  refuse({2, 4, 2, 4, 3, 1, 0}, "no output frame");
  refuse({2, 4, 3, 4, 8, 1, 4}, "no output frame");
  std::printf("dense_conv_plan_check: %d shapes accepted, %d refused, all as the header states\n", accepted, refused);
  return 0;
}
