// Internal: the owners of device resources.  Every hipMalloc / hipHostMalloc / hipEventCreate / hipStreamCreate result of the
// library lives in one of these (lh_alloc's, which the caller owns, apart): move-only, released by the destructor, on the
// device it came from.  Anything non-trivial is in dev.cpp.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <utility>

namespace lh {

// development / tests (lh_debug_live_resources, lh_debug_fail_acquire_after): how many owners hold a resource right now -
// device blocks, pinned blocks, events, streams -, and "the (n + 1)-th acquisition from now on fails, once" (n < 0: off)
void owned_live(uint64_t out[4]);
void owned_fail_acquire_after(int64_t n);

// The current HIP device is a per-host-thread setting: makes `device` current for the scope and restores the caller's.
// device < 0: nothing.  `nothrow`: for destructors and free paths - a device that cannot be made current is left alone.
struct OnDevice {
  int prev = -1;
  bool switched = false;
  explicit OnDevice(int device, bool nothrow = false);
  ~OnDevice();
  OnDevice(const OnDevice&) = delete;
  OnDevice& operator=(const OnDevice&) = delete;
};

// A device block, allocated on the device that is current and freed on that device.
class DevMem {
 public:
  DevMem() = default;
  explicit DevMem(size_t bytes) { alloc(bytes); }
  DevMem(DevMem&& o) noexcept : p_(o.p_), bytes_(o.bytes_), device_(o.device_) { o.p_ = nullptr, o.bytes_ = 0; }
  DevMem& operator=(DevMem&& o) noexcept {
    if (this != &o) reset(), p_ = o.p_, bytes_ = o.bytes_, device_ = o.device_, o.p_ = nullptr, o.bytes_ = 0;
    return *this;
  }
  ~DevMem() { reset(); }
  void alloc(size_t bytes);      // a fresh block (what it held is freed first); throws LH_ERR_DEVICE
  bool try_alloc(size_t bytes);  // the same; false when the device has no room
  // grows to at least `bytes` (a fresh block of max(bytes, min_bytes): the contents are not kept); -> get()
  void* reserve(size_t bytes, size_t min_bytes = 0) {
    if (bytes > bytes_) alloc(bytes < min_bytes ? min_bytes : bytes);
    return p_;
  }
  void reset();
  void* release() {  // the caller frees it
    void* p = p_;
    if (p) forget();
    return p;
  }
  void* get() const { return p_; }
  size_t size() const { return bytes_; }
  int device() const { return device_; }
  explicit operator bool() const { return p_ != nullptr; }
  template <class T>
  T* as() const {
    return (T*)p_;
  }
  template <class T>
  operator T*() const {  // (kernel wrappers read an owner like the pointer it holds)
    return (T*)p_;
  }

 private:
  void forget();
  void* p_ = nullptr;
  size_t bytes_ = 0;
  int device_ = -1;
};

// A pinned host block (hipHostMalloc) with the flags it is allocated with.
class PinnedMem {
 public:
  explicit PinnedMem(unsigned flags = hipHostMallocDefault) : flags_(flags) {}
  PinnedMem(PinnedMem&& o) noexcept : p_(o.p_), bytes_(o.bytes_), flags_(o.flags_) { o.p_ = nullptr, o.bytes_ = 0; }
  PinnedMem& operator=(PinnedMem&& o) noexcept {
    if (this != &o) reset(), p_ = o.p_, bytes_ = o.bytes_, flags_ = o.flags_, o.p_ = nullptr, o.bytes_ = 0;
    return *this;
  }
  ~PinnedMem() { reset(); }
  void alloc(size_t bytes);  // a fresh block (what it held is freed first); throws LH_ERR_DEVICE
  // grows to at least `bytes` (a fresh block of max(bytes, min_bytes): the contents are not kept); -> get()
  void* reserve(size_t bytes, size_t min_bytes = 0) {
    if (bytes > bytes_) alloc(bytes < min_bytes ? min_bytes : bytes);
    return p_;
  }
  void reset();
  void* get() const { return p_; }
  size_t size() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }
  template <class T>
  T* as() const {
    return (T*)p_;
  }
  template <class T>
  operator T*() const {
    return (T*)p_;
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
  unsigned flags_;
};

// An event that creates itself on the first get(), with the flags given at construction (timing by default).
class Event {
 public:
  explicit Event(unsigned flags = hipEventDefault) : flags_(flags) {}
  Event(Event&& o) noexcept : ev_(o.ev_), flags_(o.flags_) { o.ev_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) reset(), ev_ = o.ev_, flags_ = o.flags_, o.ev_ = nullptr;
    return *this;
  }
  ~Event() { reset(); }
  hipEvent_t get() {
    if (!ev_) create();
    return ev_;
  }
  bool created() const { return ev_ != nullptr; }
  void reset();

 private:
  void create();
  hipEvent_t ev_ = nullptr;
  unsigned flags_;
};

// A stream; empty until created.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) reset(), s_ = o.s_, o.s_ = nullptr;
    return *this;
  }
  ~Stream() { reset(); }
  void create(unsigned flags);
  void create(unsigned flags, int priority);
  void reset();
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace lh
