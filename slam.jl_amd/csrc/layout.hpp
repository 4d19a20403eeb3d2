// layout.hpp -- regions of one scratch / pinned block, each starting on a 256-byte boundary.  A region is named ONCE, element type and
// count together: take<T>(count) carries the offset, at(base) binds it to a block (the mapped pinned block has two bases, the host's
// and the device's: one region serves both), bytes() sizes the copies.  No HIP call: tests/c_host/pose_records_check.cpp and kfmap_ring_check.cpp include it alone.
#pragma once
#include <cstddef>
template <class T> struct Region {
    size_t off = 0, count = 0;
    T *at(char *base) const { return (T *)(base + off); }
    size_t bytes() const { return count * sizeof(T); }
};
struct Layout {
    size_t end = 0;
    size_t take(size_t bytes) { const size_t at = end; end += (bytes + 255) & ~(size_t)255; return at; }      // untyped: returns the region's offset
    template <class T> Region<T> take(size_t count) { return {take(count * sizeof(T)), count}; }
    // a region of a long-lived allocation, named once for both passes of a *_regions function: without a block (base == nullptr) it only counts towards
    // the total, with the block it also points p at the region
    template <class T> void bind(T *&p, size_t bytes, char *base) { const size_t at = take(bytes); if (base) p = (T *)(base + at); }
    size_t size() const { return end; }
};
