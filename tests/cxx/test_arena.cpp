// The scratch arena of the mesh units (field_interpolation_amd/csrc/fi_arena.h) on the host, no device: the sizing pass and
// the laying-out pass agree, pieces are 256-byte aligned and disjoint, a count of 0 or below takes one element, bytes() is the
// end of the last piece.  Every piece is filled through its own pointer and read back: built with the address and
// undefined-behaviour sanitizers (tests/test_arena.py), a piece that ran past the block or was misaligned for its type
// would stop the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fi_arena.h"

using fi::prim::Arena;

namespace {

int failures = 0;
#define CHECK(cond)                                                       \
	do {                                                                  \
		if (!(cond)) {                                                    \
			std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
			++failures;                                                   \
		}                                                                 \
	} while (0)

struct Piece {
	char*  p;
	size_t bytes;  // what the caller may use
};

struct Row {  // an odd-sized element with 8-byte alignment, as fi_mesh_part
	double a, b;
	float  c[5];
};

// the same calls for both passes; counts around the 256-byte edge, of several element sizes
template <typename T>
void take(Arena& a, int64_t count, std::vector<Piece>& out)
{
	T* p = a.take<T>(count);
	out.push_back(Piece{reinterpret_cast<char*>(p), sizeof(T) * static_cast<size_t>(count > 0 ? count : 1)});
}

void lay_out(Arena& a, std::vector<Piece>& out)
{
	for (int64_t n : {63, 64, 65}) {
		take<uint32_t>(a, n + 1, out);
		take<uint64_t>(a, n, out);
		take<uint8_t>(a, 3 * n, out);
	}
	take<uint32_t>(a, 0, out);
	take<double>(a, -5, out);
	take<char>(a, 1, out);
	take<char>(a, 255, out);
	take<char>(a, 256, out);
	take<char>(a, 257, out);
	take<Row>(a, 7, out);
	take<uint64_t>(a, 100000, out);
}

}  // namespace

int main()
{
	std::vector<Piece> sized, laid;
	Arena              sizing(nullptr);
	lay_out(sizing, sized);
	for (const Piece& s : sized) { CHECK(s.p == nullptr); }
	const size_t total = sizing.bytes();
	CHECK(total > 0 && total % 256 == 0);

	char* block = static_cast<char*>(std::aligned_alloc(256, total));  // (a device block is at least that aligned)
	CHECK(block != nullptr);
	Arena arena(block);
	lay_out(arena, laid);
	CHECK(arena.bytes() == total);
	CHECK(laid.size() == sized.size());

	// the offsets of the second pass are the running size of the first
	size_t at = 0;
	for (size_t i = 0; i < laid.size(); ++i) {
		const Piece& q = laid[i];
		CHECK(q.bytes == sized[i].bytes);
		CHECK(q.p == block + at);                                   // follows its predecessor's padded end: no overlap, no gap
		CHECK(reinterpret_cast<uintptr_t>(q.p) % 256 == 0);
		CHECK(q.p + q.bytes <= block + total);
		at += (q.bytes + 255) / 256 * 256;
		if (i + 1 < laid.size()) { CHECK(q.p + q.bytes <= laid[i + 1].p); }
	}
	CHECK(at == total);                                             // bytes(): the end of the last piece

	// a count of 0 or below: one element
	{
		Arena a(nullptr);
		(void)a.take<uint32_t>(0);
		CHECK(a.bytes() == 256);
		(void)a.take<double>(-1);
		CHECK(a.bytes() == 512);
		(void)a.take<Row>(0);
		CHECK(a.bytes() == 768);
		(void)a.take<char>(257);
		CHECK(a.bytes() == 768 + 512);
	}

	// fill every piece through its pointer, then read every piece back: nobody wrote into anybody else
	for (size_t i = 0; i < laid.size(); ++i) { std::memset(laid[i].p, static_cast<int>(i + 1), laid[i].bytes); }
	for (size_t i = 0; i < laid.size(); ++i) {
		bool same = true;
		for (size_t k = 0; k < laid[i].bytes; ++k) { same = same && static_cast<unsigned char>(laid[i].p[k]) == i + 1; }
		CHECK(same);
	}
	// a typed store to the last element of the two last pieces (the sanitizer checks its alignment and its bounds)
	reinterpret_cast<Row*>(laid[laid.size() - 2].p)[6].a        = 1.0;
	reinterpret_cast<uint64_t*>(laid.back().p)[100000 - 1]        = 1;
	std::free(block);
	if (failures == 0) { std::printf("all arena checks passed\n"); }
	return failures == 0 ? 0 : 1;
}
