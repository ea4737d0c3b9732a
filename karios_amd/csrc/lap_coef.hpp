// lap_coef.hpp: the integer taps of cv2.Laplacian's separable kernels (OpenCV getSobelKernels, order 0 / 2), one table for every
// Laplacian of the library: the dense stretch + Laplacian pass (k_lap.hip, lap_make_plan) and the key-point chips (k_chips.hip, and
// the host build of its launchers in k_chips.hpp).  Plain C++.
#pragma once

struct lap_coef {
    int kd[2][11];
    int ks[2][11];
    int b3[2] = {0, 0};      // marching kernel, radius 5: image i is kernel 11 = its 9-tap pass + a 3 x 3 binomial (lap_march_item)
};

// OpenCV getSobelKernels recurrence (order 0 / 2), centred into an 11-tap array of radius R
static inline bool fill_coef(int ksize, int R, int *kd, int *ks)
{
    int d[12] = {0}, s[12] = {0};
    auto gen = [](int k, int order, int *ker) {
        if (k == 3) {
            static const int k0[3] = {1, 2, 1}, k2[3] = {1, -2, 1};
            for (int i = 0; i < 3; i++) ker[i] = order == 0 ? k0[i] : k2[i];
            return;
        }
        ker[0] = 1;
        for (int i = 0; i < k; i++) ker[i + 1] = 0;
        for (int i = 0; i < k - order - 1; i++) {
            int oldv = ker[0];
            for (int j = 1; j <= k; j++) { int nv = ker[j] + ker[j - 1]; ker[j - 1] = oldv; oldv = nv; }
        }
        for (int i = 0; i < order; i++) {
            int oldv = -ker[0];
            for (int j = 1; j <= k; j++) { int nv = ker[j - 1] - ker[j]; ker[j - 1] = oldv; oldv = nv; }
        }
    };
    int r;
    if (ksize == 1) { d[0] = 1; d[1] = -2; d[2] = 1; s[0] = 0; s[1] = 1; s[2] = 0; r = 1; }
    else if (ksize == 3 || ksize == 5 || ksize == 7 || ksize == 9 || ksize == 11) { gen(ksize, 2, d); gen(ksize, 0, s); r = ksize / 2; }
    else return false;
    if (r > R) return false;
    for (int i = 0; i < 11; i++) { kd[i] = 0; ks[i] = 0; }
    for (int i = 0; i < 2 * r + 1; i++) { kd[i + (R - r)] = d[i]; ks[i + (R - r)] = s[i]; }
    return true;
}
