// librr.so — workspace arena.  An entry's one layout(Arena&, sizes) function both sizes its workspace
// (measuring arena: null base) and carves the caller's.  Plain C++17, no HIP: host programs include it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rr {

class Arena {
  public:
    static constexpr size_t ALIGN = 256;

    // the base is aligned up here, once; bytes() charges ALIGN for that whatever the base is
    explicit Arena(void* workspace = nullptr, size_t bytes = 0)
        : base_(workspace ? (char*)workspace + (ALIGN - (uintptr_t)workspace % ALIGN) % ALIGN : nullptr), cap_(bytes) {}

    // next ALIGN-aligned block of count * sizeof(T); nullptr when measuring or when it does not fit
    template <typename T>
    T* take(size_t count) {
        const size_t off = need_ - ALIGN;
        if (need_ == SIZE_MAX || count > (SIZE_MAX - need_ - (ALIGN - 1)) / sizeof(T)) {
            need_ = SIZE_MAX;   // saturate: never wrap
            return nullptr;
        }
        need_ += (count * sizeof(T) + ALIGN - 1) / ALIGN * ALIGN;
        return base_ && fits() ? reinterpret_cast<T*>(base_ + off) : nullptr;
    }

    size_t bytes() const { return need_; }                                // what a caller must provide
    bool fits() const { return need_ != SIZE_MAX && need_ <= cap_; }      // carving: the caller did

  private:
    char* base_;
    size_t cap_, need_ = ALIGN;
};

// the bytes a layout function asks for
template <typename Layout, typename... Sizes>
size_t measured(Layout layout, const Sizes&... sizes) {
    Arena a;
    layout(a, sizes...);
    return a.bytes();
}

}  // namespace rr
