// What the tiled conv kernels share (conv_wino.hip, conv_wino43.hip, conv_bf16p.hip): how a 1-D grid is cut into (column block,
// group of sub-blocks), the launcher's inverse of that map, and the table of a workgroup's sub-blocks.
// (conv_direct.hip cuts a frame into row tiles, rt = (li / ctiles) * 8 + xcd, in its conv_row_tile: another scheme, not this one.)
#pragma once
#include "common.h"

// Workgroup id -> (column block cb of nCB, sub-block group sp).  XCD-aware: workgroup ids go round the eight XCDs, and an XCD
// keeps one column block (nCB >= 8: one of every eight) so that its slice of the packed weights stays in that XCD's L2.  Groups
// sp >= NS exist where 8 / nCB does not divide NS: the kernel returns on them.
__host__ __device__ __forceinline__ void conv_tile_wg(int id, int nCB, int& cb, int& sp) {
    const int xcd = id & 7, slot = id >> 3;
    if (nCB >= 8) {
        const int kN = nCB >> 3;
        cb = (slot % kN) * 8 + xcd;
        sp = slot / kN;
    } else {
        const int per = 8 / nCB;
        cb = xcd % nCB;
        sp = slot * per + xcd / nCB;
    }
}

// The launcher's side of conv_tile_wg: the column-block counts the map takes, and the grid that makes it produce every
// (cb, sp < NS) exactly once.
static inline bool conv_tile_ncb_ok(int nCB) { return nCB <= 8 ? (8 % nCB) == 0 : (nCB % 8) == 0; }
static inline long long conv_tile_grid(long long NS, int nCB) {
    long long slots;                                  // workgroup ids = slots * 8
    if (nCB >= 8) slots = NS * (nCB / 8);
    else { const int per = 8 / nCB; slots = (NS + per - 1) / per; }
    return slots * 8;
}

// The sub-block table of group sp: sub-block sq = sp * NSUB + i of the batch's NQ (frame-major, then rows of byN x bxN per frame)
// -> its frame (-1 past the end) and the pixel origin of its ph x pw pixels; (by0, bx0): first sub-block row / column of a
// computed window (0, 0: whole frames).  Every thread calls it; the caller's barrier publishes the table.
template <int NSUB>
__device__ __forceinline__ void conv_tile_subblocks(int* s_sbf, int* s_sby, int* s_sbx, int tid, int sp, int NQ, int bxN, int byN,
                                                    int ph, int pw, int by0, int bx0) {
    if (tid < NSUB) {
        const int sq = sp * NSUB + tid;
        if (sq < NQ) {
            const int bx = sq % bxN;
            const int t1 = sq / bxN;
            s_sbf[tid] = t1 / byN; s_sby[tid] = ph * (by0 + t1 % byN); s_sbx[tid] = pw * (bx0 + bx);
        } else {
            s_sbf[tid] = -1; s_sby[tid] = 0; s_sbx[tid] = 0;
        }
    }
}
