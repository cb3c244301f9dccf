// Where the range kernels of events.hip take their records from: the 8-byte .dat records as they are (RawRecords) or the packed records
// of records.hip (PackedRecords; include/eas_hip.h states the format).  A source answers two questions -- is [a, e) a range to walk
// (admit), and what is logical record i (load: time, x, y, polarity; false = there is nothing to read) -- and nothing else: window rule,
// route to a bin and finishing pass are the callers'.
#pragma once
#include "eas_common.h"

struct RecEvent {
    uint32_t t, x, y, p;
};

// the fields of a .dat record: 32 bits of time, then x (14 bits), y (14 bits), polarity (1 bit); bits 29-31 carry nothing the frames read
__device__ __forceinline__ RecEvent rec_decode(uint2 v) { return RecEvent{v.x, v.y & 16383u, (v.y >> 14) & 16383u, (v.y >> 28) & 1u}; }

struct RawRecords {
    const uint2* __restrict__ rec;
    __device__ __forceinline__ bool admit(int64_t a, int64_t e) const { return e > a; }       // the caller answers for the range lying inside
    __device__ __forceinline__ bool load(int64_t i, RecEvent& ev) const {
        ev = rec_decode(rec[i]);
        return true;
    }
};

// ---- packed records: blocks of 64, a narrow block 64 words of XB + YB + 1 + DB bits, a wide block its 64 records
#define EAS_REC_BLOCK 64                 // records per block = lanes per wave
#define EAS_REC_UNIT 256                 // bytes per payload unit: a narrow block is one unit, a wide block two
#define EAS_REC_FLAG_RANGE 1u            // flag bit 0: a range outside [0, packed records) or with e < a -- walked as empty
#define EAS_REC_FLAG_TABLE 2u            // flag bit 1: a table entry whose units lie outside the payload -- its records are skipped

struct RecWidths {
    int xb, yb, db;
};
static inline int rec_bits(int v) {      // bits of v, at least 1
    int b = 1;
    while ((v >> b) != 0) ++b;
    return b;
}
// false: the geometry leaves fewer than 8 bits for the time offset (or is no geometry)
static inline bool rec_widths(int H, int W, RecWidths& w) {
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return false;
    w.xb = rec_bits(W - 1);
    w.yb = rec_bits(H - 1);
    w.db = 31 - w.xb - w.yb;
    return w.db >= 8;
}

struct PackedRecords {
    const uint2* __restrict__ table;     // [nb] (base time, unit offset | wide << 31)
    const uint8_t* __restrict__ payload; // [units] units of EAS_REC_UNIT bytes
    int64_t nb, units;
    int xb, yb;
    uint32_t* flags;                     // nullable: the word the two flag bits are set in

    __device__ __forceinline__ void flag(uint32_t bit) const {
        if (flags) atomicOr(flags, bit);
    }
    __device__ __forceinline__ bool admit(int64_t a, int64_t e) const {
        if (a < 0 || e > nb * EAS_REC_BLOCK || e < a) {
            flag(EAS_REC_FLAG_RANGE);
            return false;
        }
        return e > a;
    }
    // logical record i, 0 <= i < nb * 64, as the record it was packed from
    __device__ __forceinline__ bool record(int64_t i, uint2& v) const {
        const uint2 entry = table[i >> 6];
        const int64_t unit = entry.y & 0x7fffffffu;
        const bool wide = (entry.y >> 31) != 0;
        const int lane = (int)(i & 63);
        if (unit + (wide ? 2 : 1) > units) {
            flag(EAS_REC_FLAG_TABLE);
            return false;
        }
        if (wide) {
            v = reinterpret_cast<const uint2*>(payload + unit * EAS_REC_UNIT)[lane];
        } else {
            const uint32_t w = reinterpret_cast<const uint32_t*>(payload + unit * EAS_REC_UNIT)[lane];
            const uint32_t x = w & ((1u << xb) - 1u), y = (w >> xb) & ((1u << yb) - 1u), p = (w >> (xb + yb)) & 1u;
            v = make_uint2(entry.x + (w >> (xb + yb + 1)), x | (y << 14) | (p << 28));
        }
        return true;
    }
    __device__ __forceinline__ bool load(int64_t i, RecEvent& ev) const {
        uint2 v;
        if (!record(i, v)) return false;
        ev = rec_decode(v);
        return true;
    }
};
