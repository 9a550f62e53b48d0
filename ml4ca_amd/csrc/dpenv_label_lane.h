// dpenv_label_lane.h - a lane's place in a labelling scan's wave and the depth of its row fetch: what the scans of dpenv_label.hip (the
// pseudo-inverse and the QP law) and of dpenv_label_nn.hip (the network) share.  Defines no kernel; included inside namespace dpenv.
#ifndef DPENV_LABEL_LANE_H
#define DPENV_LABEL_LANE_H

// rows fetched ahead per register bank, two banks (score_kernel's scheme and its winner, dpenv_score_dev.h): a row is 7 loads per lane
constexpr int LABEL_U = 2;

// one wave per workgroup, one lane per env: dead lanes shadow env n - 1 (il) and store nothing
struct LabelLane {
    int lane, wave0, i, il;
    bool live;
};
__device__ __forceinline__ LabelLane label_lane(int n)
{
    LabelLane L;
    L.lane = threadIdx.x;
    L.wave0 = blockIdx.x * 64;
    L.i = L.wave0 + L.lane;
    L.live = L.i < n;
    L.il = L.live ? L.i : n - 1;
    return L;
}

#endif
