// orbx_stage.h -- where the host arrays of one call live inside ONE pinned buffer (host only: no HIP header, g++ compiles it alone).
//
// A call lists its arrays ONCE, in buffer order, with OrbxStagePlan::add(); every add() returns a typed slot that carries only the array's offset.
// OrbxCallBox / OrbxHostStage::begin() (orbx_internal.h) size their buffers from the plan's total(), copy every listed array in (fill()) and hand out an
// OrbxStaged view.  Call sites resolve a slot through that view (the buffers are then as large as the plan) or, for a copy of the buffer in device
// memory and for working arrays, with slot.in(base); resolving against the box's raw members is possible and is not done.
#ifndef ORBX_STAGE_H
#define ORBX_STAGE_H

#include <cstring>
#include <stddef.h>
#include <stdint.h>
#include <vector>

/* the call's inputs / its results / a handle's device working arrays: a slot of one side does not resolve against another (a working slot only through in()) */
enum OrbxStageSide { ORBX_STAGE_IN, ORBX_STAGE_OUT, ORBX_STAGE_WORK };

/* An array of T at `off` bytes inside a staged buffer.  in(base): the same offset inside another copy of the buffer (the device arena). */
template <typename T, OrbxStageSide SIDE> struct OrbxSlot {
    size_t off;
    T *in(void *base) const { return (T *)((uint8_t *)base + off); }
    const T *in(const void *base) const { return (const T *)((const uint8_t *)base + off); }
};

template <OrbxStageSide SIDE> struct OrbxStagePlan {
    struct Item { const void *src; size_t copy, room, off; };      /* bytes to copy from src, bytes reserved, offset */
    std::vector<Item> items;      /* kept from call to call: reset() keeps the capacity, so a warm handle allocates nothing */
    size_t sum = 0;
    static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    void reset() { items.clear(); sum = 0; }
    /* `count` elements from src into room for `room` (>= count) elements.  src == nullptr or count == 0: a hole the caller fills after begin().
     * room == 0: nothing is added and nothing moves (an absent optional array); the slot then names the offset of whatever comes next. */
    template <typename T> OrbxSlot<T, SIDE> add(const T *src, size_t count, size_t room)
    {
        const OrbxSlot<T, SIDE> s{sum};
        if (!room) return s;
        if (count > room) count = room;
        items.push_back(Item{src, src ? count * sizeof(T) : 0, room * sizeof(T), sum});
        sum += padded(room * sizeof(T));
        return s;
    }
    template <typename T> OrbxSlot<T, SIDE> add(const T *src, size_t count) { return add(src, count, count); }
    template <typename T> OrbxSlot<T, SIDE> hole(size_t room) { return add((const T *)nullptr, 0, room); }
    size_t total() const { return sum; }
    /* every listed array into a buffer of at least total() bytes */
    void fill(uint8_t *base) const
    {
        for (const Item &it : items)
            if (it.copy) memcpy(base + it.off, it.src, it.copy);
    }
};
typedef OrbxStagePlan<ORBX_STAGE_IN> OrbxInPlan;
typedef OrbxStagePlan<ORBX_STAGE_OUT> OrbxOutPlan;
typedef OrbxStagePlan<ORBX_STAGE_WORK> OrbxWorkPlan;

/* The buffers behind the plans of one begun call, from the host's and from the device's side.  Only begin() makes one. */
class OrbxStaged {
    uint8_t *inHost, *inDev, *outHost, *outDev;
    OrbxStaged(uint8_t *ih, uint8_t *id, uint8_t *oh, uint8_t *od) : inHost(ih), inDev(id), outHost(oh), outDev(od) {}
    friend struct OrbxHostStage;
    friend struct OrbxCallBox;
public:
    template <typename T> T *host(OrbxSlot<T, ORBX_STAGE_IN> s) const { return s.in(inHost); }
    template <typename T> T *dev(OrbxSlot<T, ORBX_STAGE_IN> s) const { return s.in(inDev); }      /* (kernels fill the holes of an OrbxHostStage) */
    template <typename T> const T *host(OrbxSlot<T, ORBX_STAGE_OUT> s) const { return s.in((const uint8_t *)outHost); }
    template <typename T> T *dev(OrbxSlot<T, ORBX_STAGE_OUT> s) const { return s.in(outDev); }
};

#endif
