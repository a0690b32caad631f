// Host side of the GPU-resident parameter store (kernels and rationale: gpu_ps.hip): one
// uncached allocation [params f32 | control words u64] on the owner's GPU, exported as an IPC
// handle; other processes open it (over xGMI when they run on another GPU).
//
// With sync_slots = R >= 1 (--sync_replicas) the allocation continues, 256-byte aligned, with
//   sync control region  u64 round word (round << 32) | tickets_taken
//                        u32 chunks_done, u32 R, u32 arrivals[ceil(n / 1024)]
//   R gradient slots     n f32 each (stride: the parameters' padded size)
// With sync_slots = 0 the allocation is exactly the async one.
//
// With opt_slots = 1 (--optimizer momentum: accum) or 2 (adam: m, v) the allocation ends with
// that many parameter-sized f32 planes (stride: the parameters' padded size), behind everything
// above; control word [2] records the count, which is the optimizer kind.  With opt_slots = 0
// every offset and the extent are unchanged.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>

#include "gpu_ps.h"

namespace py = pybind11;

#define GPS_CHECK(expr)                                                                \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) +     \
                               " in " #expr);                                          \
  } while (0)

namespace dtfx {

class GpuParamStore {
 public:
  // [0] global_step, [1] initialised flag, [2] opt_slots (the optimizer kind)
  static constexpr int kCtrlWords = 32;
  static constexpr int kOptWord = 2;

  // owner: allocate + zero; otherwise open(handle) before use
  GpuParamStore(int device, long long n, bool owner, int sync_slots = 0, int opt_slots = 0)
      : device_(device), n_(n), owner_(owner), sync_slots_(sync_slots), opt_slots_(opt_slots) {
    if (n < 1) throw std::runtime_error("gpu_ps: n must be >= 1");
    if (sync_slots < 0 || sync_slots > kMaxSyncSlots)
      throw std::runtime_error("gpu_ps: sync_slots must be in [0, 1024]");
    if (opt_slots < 0 || opt_slots > 2)
      throw std::runtime_error("gpu_ps: opt_slots must be 0 (sgd), 1 (momentum) or 2 (adam)");
    GPS_CHECK(hipSetDevice(device));
    pbytes_ = (n * 4 + 255) / 256 * 256;
    used_ = pbytes_ + kCtrlWords * 8;
    if (sync_slots_ > 0) {
      nchunks_ = (n + 1023) / 1024;
      sync_off_ = used_;  // 256-byte aligned: pbytes_ is, and the control block is 256 bytes
      slots_off_ = sync_off_ + (kSyncHeader + 4 * nchunks_ + 255) / 256 * 256;
      used_ = slots_off_ + (long long)sync_slots_ * pbytes_;
    }
    opt_off_ = used_;  // 256-byte aligned with or without the sync region
    used_ += (long long)opt_slots_ * pbytes_;
    bytes_ = (used_ + (2u << 20) - 1) / (2u << 20) * (2u << 20);
    if (owner) {
      GPS_CHECK(hipExtMallocWithFlags(&base_, bytes_, hipDeviceMallocUncached));
      GPS_CHECK(hipMemset(base_, 0, bytes_));
      if (opt_slots_ > 0) {
        const unsigned long long k = (unsigned long long)opt_slots_;
        GPS_CHECK(hipMemcpy(static_cast<char*>(base_) + pbytes_ + 8 * kOptWord, &k, 8,
                            hipMemcpyHostToDevice));
      }
    }
    GPS_CHECK(hipHostMalloc(&host_word_, 64, hipHostMallocDefault));
    GPS_CHECK(hipMalloc(&dev_word_, 64));
    if (sync_slots_ > 0) {
      if (owner) {  // everything else is zero: round 0, no tickets, no arrivals
        const unsigned r = (unsigned)sync_slots_;
        GPS_CHECK(hipMemcpy(static_cast<char*>(base_) + sync_off_ + 12, &r, 4,
                            hipMemcpyHostToDevice));
      }
      // staging words of the sync calls, apart from the fetch_add ones the saver thread uses
      GPS_CHECK(hipHostMalloc(&sync_host_, kSyncStage, hipHostMallocDefault));
      GPS_CHECK(hipMalloc(&sync_dev_, kSyncStage));
    }
  }
  ~GpuParamStore() { close(); }

  py::bytes handle() {
    if (!owner_ || !base_) throw std::runtime_error("gpu_ps: only the owner exports a handle");
    hipIpcMemHandle_t h;
    GPS_CHECK(hipIpcGetMemHandle(&h, base_));
    return py::bytes(reinterpret_cast<const char*>(&h), sizeof(h));
  }

  static int handle_size() { return (int)sizeof(hipIpcMemHandle_t); }

  void open(const std::string& handle) {
    if (owner_) return;
    hipIpcMemHandle_t h;
    if (handle.size() != sizeof(h)) throw std::runtime_error("gpu_ps: bad handle size");
    std::memcpy(&h, handle.data(), sizeof(h));
    GPS_CHECK(hipSetDevice(device_));
    GPS_CHECK(hipIpcOpenMemHandle(&base_, h, hipIpcMemLazyEnablePeerAccess));
    {  // the owner's optimizer must be this process's (same planes, same apply kernels)
      unsigned long long k = 0;
      GPS_CHECK(hipMemcpy(&k, static_cast<char*>(base_) + pbytes_ + 8 * kOptWord, 8,
                          hipMemcpyDeviceToHost));
      if (k != (unsigned long long)opt_slots_) {
        hipIpcCloseMemHandle(base_);
        base_ = nullptr;
        throw std::runtime_error("gpu_ps: the store was created with opt_slots = " +
                                 std::to_string(k) + ", this process asked for " +
                                 std::to_string(opt_slots_));
      }
    }
    if (sync_slots_ > 0) {  // the owner's R must be this process's (same layout, same mean)
      hipDeviceptr_t rb = nullptr;
      size_t rsize = 0;
      const bool known = hipMemGetAddressRange(&rb, &rsize, base_) == hipSuccess;
      if (!known) (void)hipGetLastError();
      unsigned r = 0;
      bool fits = !known || (long long)rsize >= used_;
      if (fits)
        GPS_CHECK(hipMemcpy(&r, static_cast<char*>(base_) + sync_off_ + 12, 4,
                            hipMemcpyDeviceToHost));
      if (!fits || r != (unsigned)sync_slots_) {
        hipIpcCloseMemHandle(base_);
        base_ = nullptr;
        throw std::runtime_error("gpu_ps: the store was created with sync_slots = " +
                                 (fits ? std::to_string(r) : std::string("0 (no sync region)")) +
                                 ", this process asked for " + std::to_string(sync_slots_));
      }
    }
  }

  uintptr_t params() const { return reinterpret_cast<uintptr_t>(base()); }
  long long numel() const { return n_; }

  void pull(uintptr_t dst, uintptr_t stream) {
    gps_pull_launch(reinterpret_cast<float*>(dst), reinterpret_cast<const float*>(base()), n_,
                    reinterpret_cast<hipStream_t>(stream));
  }

  void push_apply(uintptr_t g, float lr, bool locking, uintptr_t stream) {
    gps_apply_launch(reinterpret_cast<float*>(base()), reinterpret_cast<const float*>(g), lr, n_,
                     locking, reinterpret_cast<hipStream_t>(stream));
  }

  // async apply of the store's stateful optimizer (opt_slots = 1: momentum, h0 = mu;
  // opt_slots = 2: adam, h0 = beta1, h1 = beta2, h2 = epsilon) on the parameters and the slot
  // planes; adam's t is global_step + 1 as each block reads it
  void push_apply_opt(uintptr_t g, float lr, float h0, float h1, float h2, uintptr_t stream) {
    need_opt();
    gps_apply_opt_launch(reinterpret_cast<float*>(base()), opt_plane(0), opt_plane(1),
                         reinterpret_cast<const float*>(g), ctrl(), lr, opt_slots_, h0, h1, h2,
                         n_, reinterpret_cast<hipStream_t>(stream));
  }

  // control word `slot` += delta on the device (system-scope atomic); returns the old value
  long long fetch_add(int slot, long long delta, uintptr_t stream) {
    return fetch_add_impl(slot, delta, stream, 0, 0, nullptr);
  }

  // the same, also reading back `nextra` (<= 14) f32 words at device address `extra` in the
  // same copy: (old value, [floats])
  py::tuple fetch_add_read(int slot, long long delta, uintptr_t stream, uintptr_t extra,
                           int nextra) {
    float vals[14];
    const long long old = fetch_add_impl(slot, delta, stream, extra, nextra, vals);
    py::list l;
    for (int i = 0; i < nextra; ++i) l.append(vals[i]);
    return py::make_tuple(old, l);
  }

  // synchronous host <-> store copies (init / restore / checkpoint); offsets in bytes
  void read(uintptr_t host, long long off, long long nbytes) {
    check_range(off, nbytes);
    py::gil_scoped_release nogil;
    GPS_CHECK(hipSetDevice(device_));
    GPS_CHECK(hipMemcpy(reinterpret_cast<void*>(host), static_cast<char*>(base()) + off, nbytes,
                        hipMemcpyDeviceToHost));
  }
  void write(uintptr_t host, long long off, long long nbytes) {
    check_range(off, nbytes);
    py::gil_scoped_release nogil;
    GPS_CHECK(hipSetDevice(device_));
    GPS_CHECK(hipMemcpy(static_cast<char*>(base()) + off, reinterpret_cast<const void*>(host),
                        nbytes, hipMemcpyHostToDevice));
  }
  long long ctrl_offset() const { return pbytes_; }
  int sync_slots() const { return sync_slots_; }
  long long sync_offset() const { return need_sync(), sync_off_; }
  long long slot_offset(int k) const {
    need_sync();
    if (k < 0 || k >= sync_slots_) throw std::runtime_error("gpu_ps: bad sync slot");
    return slots_off_ + (long long)k * pbytes_;
  }
  int opt_slots() const { return opt_slots_; }
  long long opt_offset(int k) const {
    need_opt();
    if (k < 0 || k >= opt_slots_) throw std::runtime_error("gpu_ps: bad optimizer slot");
    return opt_off_ + (long long)k * pbytes_;
  }

  // global_step = step (init / restore).  On a sync-enabled store the rounds own the counter:
  // the round word becomes (step << 32) and the arrival counters are re-armed.  Not for use
  // while workers are pushing.
  void set_step(long long step) {
    if (step < 0 || (sync_slots_ > 0 && step > 0xffffffffLL))
      throw std::runtime_error("gpu_ps: global_step out of range");
    py::gil_scoped_release nogil;
    GPS_CHECK(hipSetDevice(device_));
    char* b = static_cast<char*>(base());
    const unsigned long long s = (unsigned long long)step;
    if (sync_slots_ > 0) {
      const unsigned long long w = s << 32;
      GPS_CHECK(hipMemset(b + sync_off_ + kSyncHeader, 0, 4 * nchunks_));  // arrivals
      GPS_CHECK(hipMemset(b + sync_off_ + 8, 0, 4));                       // chunks_done
      GPS_CHECK(hipMemcpy(b + pbytes_, &s, 8, hipMemcpyHostToDevice));
      GPS_CHECK(hipMemcpy(b + sync_off_, &w, 8, hipMemcpyHostToDevice));
    } else {
      GPS_CHECK(hipMemcpy(b + pbytes_, &s, 8, hipMemcpyHostToDevice));
    }
  }

  // One sync push: join (ticket of round `local_step`) + push (gradient into the ticket's slot;
  // the R-th arrival of each chunk applies p -= (lr / R) * sum) enqueued back to back, then ONE
  // read-back of the decision word and `nextra` (<= 14) f32 words at device address `extra`.
  // Returns (status, round seen, ticket, [floats]); never waits on another worker.
  // With a stateful optimizer the closer runs it on the mean (h0, h1, h2 as in push_apply_opt).
  py::tuple sync_begin(uintptr_t g, float lr, long long local_step, uintptr_t stream,
                       uintptr_t extra, int nextra, float h0, float h1, float h2) {
    need_sync();
    if (local_step < 0 || local_step > 0xffffffffLL)
      throw std::runtime_error("gpu_ps: local_step out of range");
    if (nextra < 0 || nextra > 14) throw std::runtime_error("gpu_ps: at most 14 extra words");
    unsigned dec[4];
    float vals[14];
    {
      py::gil_scoped_release nogil;
      std::lock_guard<std::mutex> lock(sync_mu_);
      const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
      enqueue_push(g, lr, local_step, s, extra, nextra, h0, h1, h2);
      GPS_CHECK(hipMemcpyAsync(sync_host_, sync_dev_, 16 + 4 * nextra, hipMemcpyDeviceToHost, s));
      GPS_CHECK(hipStreamSynchronize(s));
      std::memcpy(dec, sync_host_, 16);
      std::memcpy(vals, static_cast<char*>(sync_host_) + 16, 4 * nextra);
    }
    py::list l;
    for (int i = 0; i < nextra; ++i) l.append(vals[i]);
    return py::make_tuple((int)dec[0], (long long)dec[2], (int)dec[1], l);
  }

  // The two launches of sync_begin alone, no read-back and no stream wait: the decision stays
  // on the device and the next call overwrites it.  For timing the launches (with R = 1 every
  // push closes its round, so pushes of consecutive steps can be queued back to back).
  void sync_enqueue(uintptr_t g, float lr, long long local_step, uintptr_t stream, float h0,
                    float h1, float h2) {
    need_sync();
    if (local_step < 0 || local_step > 0xffffffffLL)
      throw std::runtime_error("gpu_ps: local_step out of range");
    py::gil_scoped_release nogil;
    std::lock_guard<std::mutex> lock(sync_mu_);
    enqueue_push(g, lr, local_step, reinterpret_cast<hipStream_t>(stream), 0, 0, h0, h1, h2);
  }

  // (round, tickets_taken): the round word through the store's 8-byte read (fetch-add of 0)
  py::tuple sync_poll(uintptr_t stream) {
    need_sync();
    unsigned long long w;
    {
      py::gil_scoped_release nogil;
      std::lock_guard<std::mutex> lock(sync_mu_);
      const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
      unsigned long long* dw = reinterpret_cast<unsigned long long*>(
          static_cast<char*>(sync_dev_) + kSyncStage / 2);
      unsigned long long* hw = reinterpret_cast<unsigned long long*>(
          static_cast<char*>(sync_host_) + kSyncStage / 2);
      gps_fetch_add_launch(round_word(), 0, dw, nullptr, 0, s);
      GPS_CHECK(hipMemcpyAsync(hw, dw, 8, hipMemcpyDeviceToHost, s));
      GPS_CHECK(hipStreamSynchronize(s));
      w = *hw;
    }
    return py::make_tuple((long long)(w >> 32), (long long)(w & 0xffffffffULL));
  }

  void close() {
    if (base_) {
      hipSetDevice(device_);
      hipDeviceSynchronize();
      if (owner_) hipFree(base_);
      else hipIpcCloseMemHandle(base_);
      base_ = nullptr;
    }
    if (host_word_) {
      hipHostFree(host_word_);
      host_word_ = nullptr;
    }
    if (dev_word_) {
      hipFree(dev_word_);
      dev_word_ = nullptr;
    }
    if (sync_host_) {
      hipHostFree(sync_host_);
      sync_host_ = nullptr;
    }
    if (sync_dev_) {
      hipFree(sync_dev_);
      sync_dev_ = nullptr;
    }
  }

 private:
  long long fetch_add_impl(int slot, long long delta, uintptr_t stream, uintptr_t extra,
                           int nextra, float* vals) {
    if (slot < 0 || slot >= kCtrlWords) throw std::runtime_error("gpu_ps: bad control slot");
    if (nextra < 0 || nextra > 14) throw std::runtime_error("gpu_ps: at most 14 extra words");
    py::gil_scoped_release nogil;
    std::lock_guard<std::mutex> lock(mu_);  // one staging buffer: the saver thread calls too
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    gps_fetch_add_launch(ctrl() + slot, delta, dev_word_, reinterpret_cast<const float*>(extra),
                         nextra, s);
    GPS_CHECK(hipMemcpyAsync(host_word_, dev_word_, 8 + 4 * nextra, hipMemcpyDeviceToHost, s));
    GPS_CHECK(hipStreamSynchronize(s));
    if (vals) std::memcpy(vals, host_word_ + 1, 4 * nextra);
    return (long long)*host_word_;
  }

  void* base() const {
    if (!base_) throw std::runtime_error("gpu_ps: store not allocated / opened");
    return base_;
  }
  unsigned long long* ctrl() const {
    return reinterpret_cast<unsigned long long*>(static_cast<char*>(base()) + pbytes_);
  }
  void check_range(long long off, long long nbytes) const {
    if (off < 0 || nbytes < 0 || off + nbytes > used_)
      throw std::runtime_error("gpu_ps: copy out of range");
  }
  // join + push on `s` (sync_mu_ held: one decision word per store object)
  void enqueue_push(uintptr_t g, float lr, long long local_step, hipStream_t s, uintptr_t extra,
                    int nextra, float h0, float h1, float h2) {
    char* b = static_cast<char*>(base());
    unsigned* d = reinterpret_cast<unsigned*>(sync_dev_);
    gps_sync_join_launch(round_word(), (unsigned)local_step, (unsigned)sync_slots_, d,
                         reinterpret_cast<const float*>(extra), nextra, s);
    gps_sync_push_launch(reinterpret_cast<float*>(b), reinterpret_cast<float*>(b + slots_off_),
                         pbytes_ / 4, reinterpret_cast<const float*>(g), d,
                         reinterpret_cast<unsigned*>(b + sync_off_ + kSyncHeader),
                         reinterpret_cast<unsigned*>(b + sync_off_ + 8), round_word(), ctrl(), lr,
                         (unsigned)sync_slots_, n_, opt_slots_, opt_plane(0), opt_plane(1), h0,
                         h1, h2, s);
  }
  void need_opt() const {
    if (opt_slots_ < 1) throw std::runtime_error("gpu_ps: the store has no optimizer slots");
  }
  float* opt_plane(int k) const {
    if (k >= opt_slots_) return nullptr;
    return reinterpret_cast<float*>(static_cast<char*>(base()) + opt_off_ + (long long)k * pbytes_);
  }
  void need_sync() const {
    if (sync_slots_ < 1) throw std::runtime_error("gpu_ps: the store has no sync slots");
  }
  unsigned long long* round_word() const {
    return reinterpret_cast<unsigned long long*>(static_cast<char*>(base()) + sync_off_);
  }

  static constexpr int kMaxSyncSlots = 1024;
  static constexpr long long kSyncHeader = 16;  // round word, chunks_done, R
  static constexpr int kSyncStage = 256;        // [decision + record | poll word]

  int device_;
  long long n_;
  bool owner_;
  int sync_slots_ = 0, opt_slots_ = 0;
  long long pbytes_ = 0, bytes_ = 0, used_ = 0;
  long long nchunks_ = 0, sync_off_ = 0, slots_off_ = 0, opt_off_ = 0;
  void* sync_host_ = nullptr;
  void* sync_dev_ = nullptr;
  std::mutex sync_mu_;
  void* base_ = nullptr;
  unsigned long long* host_word_ = nullptr;
  unsigned long long* dev_word_ = nullptr;
  std::mutex mu_;
};

}  // namespace dtfx

void register_gpu_ps(py::module_& m) {
  py::class_<dtfx::GpuParamStore>(m, "GpuParamStore")
      .def(py::init<int, long long, bool, int, int>(), py::arg("device"), py::arg("n"),
           py::arg("owner"), py::arg("sync_slots") = 0, py::arg("opt_slots") = 0)
      .def("handle", &dtfx::GpuParamStore::handle)
      .def_static("handle_size", &dtfx::GpuParamStore::handle_size)
      .def("open", &dtfx::GpuParamStore::open)
      .def("params", &dtfx::GpuParamStore::params)
      .def("numel", &dtfx::GpuParamStore::numel)
      .def("pull", &dtfx::GpuParamStore::pull, py::arg("dst"), py::arg("stream"))
      .def("push_apply", &dtfx::GpuParamStore::push_apply, py::arg("g"), py::arg("lr"),
           py::arg("locking"), py::arg("stream"))
      .def("push_apply_opt", &dtfx::GpuParamStore::push_apply_opt, py::arg("g"), py::arg("lr"),
           py::arg("h0"), py::arg("h1"), py::arg("h2"), py::arg("stream"))
      .def("fetch_add", &dtfx::GpuParamStore::fetch_add, py::arg("slot"), py::arg("delta"),
           py::arg("stream"))
      .def("fetch_add_read", &dtfx::GpuParamStore::fetch_add_read, py::arg("slot"),
           py::arg("delta"), py::arg("stream"), py::arg("extra"), py::arg("nextra"))
      .def("read", &dtfx::GpuParamStore::read)
      .def("write", &dtfx::GpuParamStore::write)
      .def("ctrl_offset", &dtfx::GpuParamStore::ctrl_offset)
      .def("sync_slots", &dtfx::GpuParamStore::sync_slots)
      .def("sync_offset", &dtfx::GpuParamStore::sync_offset)
      .def("slot_offset", &dtfx::GpuParamStore::slot_offset)
      .def("opt_slots", &dtfx::GpuParamStore::opt_slots)
      .def("opt_offset", &dtfx::GpuParamStore::opt_offset)
      .def("set_step", &dtfx::GpuParamStore::set_step, py::arg("step"))
      .def("sync_begin", &dtfx::GpuParamStore::sync_begin, py::arg("grad"), py::arg("lr"),
           py::arg("local_step"), py::arg("stream"), py::arg("extra"), py::arg("nextra"),
           py::arg("h0") = 0.f, py::arg("h1") = 0.f, py::arg("h2") = 0.f)
      .def("sync_enqueue", &dtfx::GpuParamStore::sync_enqueue, py::arg("grad"), py::arg("lr"),
           py::arg("local_step"), py::arg("stream"), py::arg("h0") = 0.f, py::arg("h1") = 0.f,
           py::arg("h2") = 0.f)
      .def("sync_poll", &dtfx::GpuParamStore::sync_poll, py::arg("stream"))
      .def("close", &dtfx::GpuParamStore::close);
}
