// mjb_resources.h — move-only owners of what a batch holds on the device (mjb_api.hip): a device buffer, a pinned host buffer, a stream, an event.
// Each frees what it holds when it is reset, assigned to or destroyed, and counts itself in g_live_resources while it holds something
// (mjb_debug_live_resources).  The raw HIP calls that create and release these four kinds of resource appear here and nowhere else in the batch code.
// The device the resource lives on must be current (hipSetDevice) around every call, the destructor included.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <utility>

#pragma GCC visibility push(hidden)

inline std::atomic<int> g_live_resources{ 0 };

template <typename T> class DevBuf {
	T *p_ = nullptr;

public:
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
	DevBuf &operator=(DevBuf &&o) noexcept
	{
		if (this != &o) {
			reset();
			p_ = std::exchange(o.p_, nullptr);
		}
		return *this;
	}
	~DevBuf() { reset(); }
	// n elements (at least one) of undefined contents, for a site that overwrites the whole buffer itself.  false: the allocation failed, the buffer is empty
	bool alloc(size_t n)
	{
		reset();
		void *p = nullptr;
		if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) {
			(void)hipGetLastError();
			return false;
		}
		p_ = static_cast<T *>(p);
		g_live_resources++;
		return true;
	}
	// ... all zero, and zero WHEN THIS RETURNS: the memset runs on the null stream, which the batches' non-blocking streams do not wait for
	bool alloc_zeroed(size_t n)
	{
		if (!alloc(n)) return false;
		if (hipMemset(p_, 0, (n ? n : 1) * sizeof(T)) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
			(void)hipGetLastError();
			reset();
		}
		return p_ != nullptr;
	}
	void reset()
	{
		if (!p_) return;
		hipFree(p_);
		p_ = nullptr;
		g_live_resources--;
	}
	T *get() const { return p_; }
	explicit operator bool() const { return p_ != nullptr; }
};

template <typename T> class PinnedBuf {
	T *p_ = nullptr;

public:
	PinnedBuf() = default;
	PinnedBuf(PinnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
	PinnedBuf &operator=(PinnedBuf &&o) noexcept
	{
		if (this != &o) {
			reset();
			p_ = std::exchange(o.p_, nullptr);
		}
		return *this;
	}
	~PinnedBuf() { reset(); }
	bool alloc_zeroed(size_t n)
	{
		reset();
		void *p = nullptr;
		if (hipHostMalloc(&p, (n ? n : 1) * sizeof(T), hipHostMallocDefault) != hipSuccess) {
			(void)hipGetLastError();
			return false;
		}
		p_ = static_cast<T *>(p);
		for (size_t i = 0; i < (n ? n : 1); i++) p_[i] = T{};
		g_live_resources++;
		return true;
	}
	void reset()
	{
		if (!p_) return;
		hipHostFree(p_);
		p_ = nullptr;
		g_live_resources--;
	}
	T *get() const { return p_; }
	explicit operator bool() const { return p_ != nullptr; }
};

// a non-blocking stream of the batch's own, or a caller's stream it only borrows (mjb_set_stream): that one is neither counted nor destroyed
class Stream {
	hipStream_t s_ = nullptr;
	bool own_ = false;

public:
	Stream() = default;
	Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)), own_(std::exchange(o.own_, false)) {}
	Stream &operator=(Stream &&o) noexcept
	{
		if (this != &o) {
			reset();
			s_ = std::exchange(o.s_, nullptr);
			own_ = std::exchange(o.own_, false);
		}
		return *this;
	}
	~Stream() { reset(); }
	hipError_t create()
	{
		reset();
		const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
		if (e != hipSuccess) {
			s_ = nullptr;
			return e;
		}
		own_ = true;
		g_live_resources++;
		return hipSuccess;
	}
	void borrow(hipStream_t s)
	{
		reset();
		s_ = s;
	}
	void reset()
	{
		if (own_) {
			hipStreamDestroy(s_);
			g_live_resources--;
		}
		s_ = nullptr;
		own_ = false;
	}
	hipStream_t get() const { return s_; }
	explicit operator bool() const { return s_ != nullptr; }
};

class Event {
	hipEvent_t e_ = nullptr;

public:
	Event() = default;
	Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
	Event &operator=(Event &&o) noexcept
	{
		if (this != &o) {
			reset();
			e_ = std::exchange(o.e_, nullptr);
		}
		return *this;
	}
	~Event() { reset(); }
	// (ordering events carry no timestamps; mjb_time_steps asks for hipEventDefault)
	hipError_t create(unsigned flags = hipEventDisableTiming)
	{
		reset();
		const hipError_t e = hipEventCreateWithFlags(&e_, flags);
		if (e != hipSuccess) {
			e_ = nullptr;
			return e;
		}
		g_live_resources++;
		return hipSuccess;
	}
	void reset()
	{
		if (!e_) return;
		hipEventDestroy(e_);
		e_ = nullptr;
		g_live_resources--;
	}
	hipEvent_t get() const { return e_; }
	explicit operator bool() const { return e_ != nullptr; }
};

#pragma GCC visibility pop
