// fi_stage.h -- the memory boundary of a call.  Every entry point takes `memory`: with FI_DEVICE a unit works on the caller's
// pointers; with FI_HOST a device copy stands in for each buffer, inputs are uploaded on the call's stream and outputs are
// copied back before the call's final stream synchronise.  A null optional buffer stays null.  Two forms, one vocabulary:
// In / Out own a DevBuf each (the query units), in / out / work / back are pieces of the call's arena (fi_arena.h).  Nothing
// here synchronises; only call-scoped buffers pass through it (objects that outlive the call copy for themselves).
#pragma once

#include "fi_arena.h"
#include "fi_internal.h"

namespace fi {

inline void check_memory(int memory)
{
	FI_REQUIRE(memory == FI_HOST || memory == FI_DEVICE, FI_ERR_INVALID, "bad memory kind %d", memory);
}

namespace stage {

// a device copy stands in for the caller's buffers
inline bool staged(int memory) { return memory == FI_HOST; }

template <typename T>
inline void upload(T* dev, const T* src, int64_t count, hipStream_t st)
{
	FI_HIP_TRY(hipMemcpyAsync(dev, src, sizeof(T) * count, hipMemcpyHostToDevice, st));
}

// an input of `count` elements on the device: the caller's pointer, or a copy uploaded on st; a null source gives null
template <typename T>
struct In {
	const T* dev;
	DevBuf   buf;
	In(const T* src, int64_t count, int memory, hipStream_t st) : dev(src)
	{
		if (!src || !staged(memory)) { return; }
		buf.alloc(sizeof(T) * count);
		upload(buf.as<T>(), src, count, st);
		dev = buf.as<T>();
	}
	operator const T*() const { return dev; }
};

// an output of `count` elements on the device: the caller's buffer, or a stand-in that back() copies to it (the first
// `upto` elements, all of them by default); a null output gives null and copies nothing
template <typename T>
struct Out {
	T*      host;
	T*      dev;
	int64_t count;
	DevBuf  buf;
	Out(T* out, int64_t n, int memory) : host(nullptr), dev(out), count(n)
	{
		if (!out || !staged(memory)) { return; }
		host = out;
		buf.alloc(sizeof(T) * count);
		dev = buf.as<T>();
	}
	void back(hipStream_t st, int64_t upto = -1)
	{
		if (host) { FI_HIP_TRY(hipMemcpyAsync(host, dev, sizeof(T) * (upto < 0 ? count : upto), hipMemcpyDeviceToHost, st)); }
	}
	operator T*() const { return dev; }
};

// ---- the same as pieces of the call's arena: called inside the lay-out lambda of prim::arena_alloc, which runs twice ----

// an input: the caller's pointer, or a piece; the pass that has the block enqueues the upload (none for a null source or a
// zero count)
template <typename T>
inline const T* in(prim::Arena& ar, const T* src, int64_t count, int memory, hipStream_t st)
{
	if (!src || !staged(memory)) { return src; }
	T* piece = ar.take<T>(count);
	if (piece && count > 0) { upload(piece, src, count, st); }
	return piece;
}

// an output: the caller's pointer, or a piece that back() copies to it; a null output gives null
template <typename T>
inline T* out(prim::Arena& ar, T* dst, int64_t count, int memory)
{
	return dst && staged(memory) ? ar.take<T>(count) : dst;
}

// an output that doubles as the working buffer, never null: the caller's device buffer where there is one, else a piece
template <typename T>
inline T* work(prim::Arena& ar, T* dst, int64_t count, int memory)
{
	return dst && !staged(memory) ? dst : ar.take<T>(count);
}

// `count` elements of a staged output back to the caller's `dst` (a null dst: nothing)
template <typename T>
inline void back(T* dst, const T* dev, int64_t count, int memory, hipStream_t st)
{
	if (dst && staged(memory)) { FI_HIP_TRY(hipMemcpyAsync(dst, dev, sizeof(T) * count, hipMemcpyDeviceToHost, st)); }
}

}  // namespace stage
}  // namespace fi
