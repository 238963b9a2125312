// carve.h -- how a block of memory (a device pool, a pinned staging block) is cut into typed pieces.  Host-only, plain C++: offset
// arithmetic with the element type attached, nothing is allocated.  A layout is a struct of pieces filled by one Carve in the order
// the pieces lie in the block (dev_layout.h holds those a host compile can see); its users call piece.in(base) on the pinned copy
// and on the device copy of the block alike.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mpa {

// n elements of T at byte `off` of a block.  An empty piece (n == 0) is legal: it marks a place and takes no room.
template<typename T> struct Piece {
	size_t off = 0, n = 0;
	T *in(void *base) const { return (T*)((char*)base + off); }
	const T *in(const void *base) const { return (const T*)((const char*)base + off); }
	size_t bytes() const { return n * sizeof(T); }
	size_t end() const { return off + bytes(); }
	// a piece inside this one (a deliberate alias: two views of one range, or what is written where something else has died)
	template<typename U> Piece<U> sub(size_t byte_off, size_t n_) const { return Piece<U>{ off + byte_off, n_ }; }
};

// Pieces back to back, each starting on a multiple of `align` (a power of two): 256 for the device pools, 64 and 16 for the upload
// blocks, 1 for the packed download blocks.  `at` is the running end: after the last piece, the size of the block.
struct Carve {
	size_t align, at = 0;
	explicit Carve(size_t align_ = 256) : align(align_) {}
	// n elements of T and extra_bytes of slack behind them
	template<typename T> Piece<T> take(size_t n, size_t extra_bytes = 0)
	{
		const Piece<T> p{ at, n };
		at += (n * sizeof(T) + extra_bytes + align - 1) & ~(align - 1);
		return p;
	}
	// an optional part: absent, it is an empty piece where it would have been
	template<typename T> Piece<T> take_if(bool cond, size_t n, size_t extra_bytes = 0) { return cond ? take<T>(n, extra_bytes) : Piece<T>{ at, 0 }; }
	void skip(size_t bytes) { at += bytes; }      // room that is no piece (the tables in front of an upload block)
};

} // namespace mpa
