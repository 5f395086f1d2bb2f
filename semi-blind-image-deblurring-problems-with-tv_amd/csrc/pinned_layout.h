// One description of a pinned staging block: the drivers add their fields in order, ask pinned_get for bytes(), and take
// every field's pointer from the block's host base and from its device view.  No driver computes a pinned offset by hand.
// Host-only arithmetic (no HIP include): tests/host_sanitize.cpp runs it under ASan.
#pragma once
#include <cstddef>

namespace sbtv {

// a field of `count` elements of T at byte offset `off` of the block
template <class T>
struct PinnedField {
    size_t off = 0, count = 0;
    // the field as seen from `base`: the block's host address or its device view
    T *at(void *base) const { return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + off); }
};

class PinnedLayout {
    size_t bytes_ = 0;

public:
    // the next field, aligned to its type
    template <class T>
    PinnedField<T> add(size_t count) {
        bytes_ = (bytes_ + alignof(T) - 1) / alignof(T) * alignof(T);
        const PinnedField<T> f{bytes_, count};
        bytes_ += sizeof(T) * count;
        return f;
    }
    size_t bytes() const { return bytes_; }
};

}  // namespace sbtv
