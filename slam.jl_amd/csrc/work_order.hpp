// work_order.hpp -- the order in which the tracking kernel visits a stream's keypoints (k_kpset_worklist, kpset.hip).
//
// Planes are column-major (a 128-byte line holds 16 rows of one column), and every keypoint's window is one wave's work in
// k_kpset_match: two keypoints share lines of their windows when they are close in x AND their rows overlap, and they share
// them in L2 only when they run close together in time.  The work list is therefore sorted by
//     (x-band, row, slot)        x-band = floor(x) / band  (band in pixels),  row = floor(y)
// so that a stream's segment walks the image band by band, top to bottom.  Ties end on the slot index: the order is a pure
// function of the list.  Shared by the kernel, the host (the stand-alone check tests/c_host/work_key_check.cpp) and nothing else.
#pragma once
#include <cstdint>

// (both branches are built: the library by hipcc, the stand-alone check by the host compiler alone)
#if defined(__HIPCC__)
#define WORK_HD __host__ __device__ __forceinline__
#else
#define WORK_HD static inline
#endif

// largest pixel coordinate a key distinguishes: both fields of the key are 16 bits wide
#define WORK_KEY_MAX_PX 65535

// floor(v) clamped to [0, hi] without ever converting a value an int cannot hold (that conversion is undefined behaviour):
// NaN -> hi (such keypoints sort last in their field), -inf and everything below 1 -> 0, +inf and everything from hi on -> hi.
WORK_HD uint32_t work_clamp_px(double v, int hi)
{
    const uint32_t top = (uint32_t)(hi < 0 ? 0 : hi > WORK_KEY_MAX_PX ? WORK_KEY_MAX_PX : hi);
    if (v != v) return top;
    if (!(v >= 1.0)) return 0;
    if (v >= (double)top) return top;
    return (uint32_t)v;                                          // 1 <= v < top <= 65535
}

// the sort key of a keypoint at (y, x) in an H x W image; band >= 1
WORK_HD uint32_t work_key(double y, double x, int H, int W, int band)
{
    return ((work_clamp_px(x, W) / (uint32_t)(band < 1 ? 1 : band)) << 16) | work_clamp_px(y, H);
}

// ---- where the work records live (KpWorkRec, kpset.hpp) ---------------------------------------------------------------------------------
// k_kpset_match deals its workgroups round-robin to the WORK_XCDS chips of the package (workgroup b runs on XCD b % 8) and gives each one
// contiguous eighth of the list: with per = ceil(ntot / 8), XCD x walks the entries [x per, min((x + 1) per, ntot)).  The records are laid out
// for that walk: 8 rows of `stride` = ceil(S cap / 8) records (>= per for every list the set can hold), entry idx in row idx / per at column
// idx % per.  Workgroup b's first record is then at (b % 8) stride + b / 8 -- kernel arguments and the workgroup index alone, so its fetch does
// not wait for ntot -- and the entry is valid iff its column r < per and (b % 8) per + r < ntot.  Slots no entry maps to hold stale bytes: they
// lie inside the 8 x stride records and are never interpreted.
#define WORK_XCDS 8
WORK_HD int work_rec_stride(long long slots) { return (int)((slots + WORK_XCDS - 1) / WORK_XCDS); }             // slots = S x cap
WORK_HD int work_rec_per(int ntot) { return (ntot + WORK_XCDS - 1) / WORK_XCDS; }
// entry idx (0 <= idx < ntot, per = work_rec_per(ntot) >= 1) -> record slot, < 8 stride
WORK_HD int work_rec_slot(int idx, int per, int stride) { return (idx / per) * stride + idx % per; }
// the inverse as the match kernel applies it: row x (0 .. 7), column r -> entry, or -1 where the slot holds none
WORK_HD int work_rec_entry(int x, int r, int per, int ntot) { return r < per && x * per + r < ntot ? x * per + r : -1; }

// Which instantiation of the tracking kernels (lk.hip: 3, 6 or 9 template slots per lane) a window_size runs on: the smallest
// whose 64 lanes hold the (2 w + 1)^2 window elements, the 9-slot one (uncached path) beyond.  The host launches by lk_slots,
// lk_level decides `cached` from the same element count.
WORK_HD int lk_window_elems(int window) { return (2 * window + 1) * (2 * window + 1); }
WORK_HD int lk_slots(int window) { const int ne = lk_window_elems(window); return ne <= 192 ? 3 : ne <= 384 ? 6 : 9; }
