// Host only: the bump allocator of the memory planners (composite.hip: a layer's buffers; model.hip: a whole pass).
#pragma once

namespace i3d {

struct Bump {           // over a caller-provided float buffer; base == null: sizing pass (every take is null, `used` counts)
    float* base;
    long used = 0;
    explicit Bump(float* b) : base(b) {}
    float* here() const { return base ? base + used : nullptr; }
    float* take(long n) {       // rounded to 4 floats: every buffer is 16-byte aligned relative to the base
        float* p = here();
        used += (n + 3) & ~3L;
        return p;
    }
};

}  // namespace i3d
