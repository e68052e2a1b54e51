// fi_arena.h -- every temporary of a call as a piece of one block.  A call of a mesh unit makes up to thirty temporaries, and
// thirty device allocations and releases cost several times what its kernels do (profiles/simplify.md).  A first pass with
// no block adds the sizes up; the same take() calls over the block of that size then hand out the pieces.  Pieces are
// 256-byte aligned; nothing lies between one piece's bytes and the next piece but that padding.
// (Plain C++, no device call: tests/cxx/test_arena.cpp checks it on the host.)
#pragma once

#include <cstddef>
#include <cstdint>

namespace fi {
namespace prim {

class Arena {
	char*  base_;
	size_t used_ = 0;

public:
	explicit Arena(void* base) : base_(static_cast<char*>(base)) {}
	template <typename T>
	T* take(int64_t count)  // (a count of 0 or below takes one element)
	{
		T* p = base_ ? reinterpret_cast<T*>(base_ + used_) : nullptr;
		used_ += (sizeof(T) * static_cast<size_t>(count > 0 ? count : 1) + 255) & ~size_t(255);
		return p;
	}
	size_t bytes() const { return used_; }
};

}  // namespace prim
}  // namespace fi
