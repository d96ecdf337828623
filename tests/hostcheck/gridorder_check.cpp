// TEST-ONLY host build of dicp_amd/csrc/dicp_gridknn.h (g++, no GPU): the density plan of a cloud and the cell key of each of its rows,
// as the grid build computes them (gknn_plan_kernel, ball_keys_kernel), for tests/normals_grid_model.py.  Never loaded by dicp_amd.
#include <algorithm>

#include "../../dicp_amd/csrc/dicp_gridknn.h"

using namespace dicp;

namespace {

// key (m): the cell key of every row, BALL_NO_KEY for the rows that stay out of the grid (at or past mb, or a non-finite coordinate);
// plan: [0] live rows, [1] flat, [2..4] the last cell per axis, [5] wy, [6] wz; edge: [0] the starting edge, [1..3] the cell edges
template <typename T>
void run(const T* y, int m, int cy, int mb, uint64_t* key, int64_t* plan, double* edge) {
    T mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    int cnt = 0;
    auto finite = [&](int j) { const T* p = y + (size_t)j * cy; return ball_finite(p[0]) && ball_finite(p[1]) && ball_finite(p[2]); };
    for (int j = 0; j < mb && j < m; ++j) {
        if (!finite(j)) continue;
        const T* p = y + (size_t)j * cy;
        for (int d = 0; d < 3; ++d) {
            mn[d] = cnt ? std::min(mn[d], p[d]) : p[d];
            mx[d] = cnt ? std::max(mx[d], p[d]) : p[d];
        }
        ++cnt;
    }
    const BallPlan<T> P = gknn_plan<T>(mn, mx, cnt);
    for (int j = 0; j < m; ++j) {
        const T* p = y + (size_t)j * cy;
        key[j] = (j < mb && P.cnt > 0 && finite(j)) ? ball_point_key(P, p[0], p[1], p[2]) : BALL_NO_KEY;
    }
    plan[0] = P.cnt; plan[1] = P.flat; plan[5] = P.wy; plan[6] = P.wz;
    edge[0] = (double)P.R;
    for (int d = 0; d < 3; ++d) { plan[2 + d] = P.hi[d]; edge[1 + d] = (double)P.s[d]; }
}

}  // namespace

extern "C" {

void go_keys_f32(const float* y, int m, int cy, int mb, uint64_t* key, int64_t* plan, double* edge) { run<float>(y, m, cy, mb, key, plan, edge); }
void go_keys_f64(const double* y, int m, int cy, int mb, uint64_t* key, int64_t* plan, double* edge) { run<double>(y, m, cy, mb, key, plan, edge); }

}
