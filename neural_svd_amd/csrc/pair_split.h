// The partition rule of the two-sided matrix-free kernel products (rbf_apply_pair.hip, dot_apply_pair.hip): a
// workgroup owns a run of 64-row x tiles (a row group) and a run of slices of at most PAIR_SLICE 64-row y chunks (a
// column group). Restated by tests/_pair_oracle.py:pair_split.
#pragma once

constexpr int PAIR_SLICE = 4;        // y chunks per slice (K^T f accumulator tiles per wave)
constexpr int PAIR_MAX_GROUPS = 32;  // partial copies of either output
constexpr int PAIR_FILL = 512;       // workgroups wanted: two per CU

// RG row groups of x tiles, CG column groups of slices: split whichever side has more work per group until the grid
// fills the chip or both sides are at one item per group / PAIR_MAX_GROUPS
inline void pair_split(int xtiles, int slices, int ltiles, int* RG, int* CG) {
    int rg = 1, cg = 1;
    const int rmax = xtiles < PAIR_MAX_GROUPS ? xtiles : PAIR_MAX_GROUPS;
    const int cmax = slices < PAIR_MAX_GROUPS ? slices : PAIR_MAX_GROUPS;
    while ((long)ltiles * rg * cg < PAIR_FILL) {
        const bool can_r = 2 * rg <= rmax, can_c = 2 * cg <= cmax;
        if (!can_r && !can_c) break;
        if (can_r && (!can_c || (long)xtiles * cg >= (long)slices * rg)) rg *= 2;
        else cg *= 2;
    }
    *RG = rg;
    *CG = cg;
}
