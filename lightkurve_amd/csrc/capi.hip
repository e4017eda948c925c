// capi.hip — extern "C" boundary of liblkhip.so (declared in include/lkhip.h).
// Host-pointer entry points stage caller buffers into HBM through StagedCall (h->staging), run the same launchers as the
// device-pointer entry points on the null stream and copy the results back; the device-pointer entry points only
// validate and enqueue kernels.  Every launcher declares its device scratch once as a lk::Scratch plan (lk_common.hpp;
// carve() is defined here, next to the Arena it carves) — h->ws for the kernels, h->staging for the double buffers of the
// chunked LS 'fast' host pipeline.
#include "lk_common.hpp"

namespace lk {

static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

int Arena::reserve(size_t bytes) {
    if (bytes <= cap) return LK_OK;
    if (used != 0) {
        set_error("Arena::reserve while sub-allocations are live");
        return LK_EHIP;
    }
    if (base) (void)hipFree(base);
    base = nullptr;
    cap = 0;
    size_t want = bytes + (bytes >> 3) + 4096;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), want);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        base = nullptr;
        return e == hipErrorOutOfMemory ? LK_ENOMEM : LK_EHIP;
    }
    cap = want;
    return LK_OK;
}

int HostStage::copy(void *dst, const void *src, size_t bytes, hipStream_t stream) {
    const int s = next;
    next = (next + 1) % SLOTS;
    if (ev[s]) LK_HIP_CHECK(hipEventSynchronize(ev[s]));  // the copy that last used this slot has finished
    if (cap[s] < bytes) {
        if (buf[s]) (void)hipHostFree(buf[s]);
        buf[s] = nullptr;
        cap[s] = 0;
        LK_HIP_CHECK(hipHostMalloc(&buf[s], bytes + 4096, hipHostMallocDefault));
        cap[s] = bytes + 4096;
    }
    if (!ev[s]) LK_HIP_CHECK(hipEventCreateWithFlags(&ev[s], hipEventDisableTiming));
    memcpy(buf[s], src, bytes);
    LK_HIP_CHECK(hipMemcpyAsync(dst, buf[s], bytes, hipMemcpyHostToDevice, stream));
    LK_HIP_CHECK(hipEventRecord(ev[s], stream));
    return LK_OK;
}

void HostStage::release() {
    for (int s = 0; s < SLOTS; ++s) {
        if (ev[s]) {
            (void)hipEventSynchronize(ev[s]);
            (void)hipEventDestroy(ev[s]);
        }
        if (buf[s]) (void)hipHostFree(buf[s]);
        buf[s] = nullptr;
        ev[s] = nullptr;
        cap[s] = 0;
    }
}

void Arena::release() {
    if (base) (void)hipFree(base);
    base = nullptr;
    cap = used = 0;
}

int Scratch::carve(hipStream_t stream) {
    if (n_ > MAX_BUFS) {
        set_error("internal: a scratch plan declares %d buffers (at most %d)", n_, MAX_BUFS);
        return LK_EHIP;
    }
    size_t total = 0;
    for (int i = 0; i < n_; ++i) total += Arena::round(bufs_[i].bytes);
    arena_.reset();
    // at least one byte: a zero-length buffer still gets a non-null pointer
    int rc = arena_.reserve(std::max<size_t>(total, 1));
    if (rc) return rc;
    void *dev[MAX_BUFS];
    for (int i = 0; i < n_; ++i)
        if (!(dev[i] = arena_.alloc(bufs_[i].bytes))) {
            arena_.reset();
            set_error("internal: scratch plan of %zu bytes does not fit its own reservation", total);
            return LK_EHIP;
        }
    for (int i = 0; i < n_; ++i) bufs_[i].set(bufs_[i].slot, dev[i]);
    for (int i = 0; i < n_; ++i)
        if (bufs_[i].src && (rc = h_->stage.copy(dev[i], bufs_[i].src, bufs_[i].bytes, stream))) return rc;
    return LK_OK;
}

// The device mirrors of one host-pointer call, in h->staging.  The call declares its buffers in carving order: in() is
// copied to the device by stage(), out() back to the host by finish(), scratch() is device-only; a null host pointer
// declares nothing and leaves its device pointer null.  stage() resets the arena, reserves exactly the declared buffers
// at Arena::alloc's 256-byte alignment, sets the device pointers and copies the inputs in.  The copies are synchronous
// and the launch between stage() and finish() goes on the null stream, so finish() reads what the kernels wrote.
class StagedCall {
  public:
    explicit StagedCall(lk_handle *h) : h_(h) {}
    // n elements copied in, n + pad on the device (the pad is left unwritten)
    template <class T> StagedCall &in(const T *&dev, const T *host, size_t n, size_t pad = 0) {
        return host ? add(dev, host, nullptr, n + pad, n, nullptr) : none(dev);
    }
    // n elements on the device, copied back: all of them, or the first *n_back (a count the launch reports)
    template <class T> StagedCall &out(T *&dev, T *host, size_t n, const int64_t *n_back = nullptr) {
        return host ? add(dev, nullptr, host, n, n, n_back) : none(dev);
    }
    template <class T> StagedCall &scratch(T *&dev, size_t n) { return add(dev, nullptr, nullptr, n, 0, nullptr); }

    int stage() {
        size_t total = 0;
        for (const Buf &b : bufs_) total += Arena::round(b.elem * b.n_dev);
        h_->staging.reset();
        // at least one byte: a zero-length buffer still gets a non-null pointer (launchers reject NULL before sizes)
        int rc = h_->staging.reserve(std::max<size_t>(total, 1));
        if (rc) return rc;
        for (Buf &b : bufs_) {
            b.dev = h_->staging.alloc(b.elem * b.n_dev);
            b.set(b.slot, b.dev);
            if (b.src) LK_HIP_CHECK(hipMemcpy(b.dev, b.src, b.elem * b.n_copy, hipMemcpyHostToDevice));
        }
        return LK_OK;
    }
    int finish() {
        for (const Buf &b : bufs_)
            if (b.dst)
                LK_HIP_CHECK(hipMemcpy(b.dst, b.dev, b.elem * (b.n_back ? (size_t)*b.n_back : b.n_copy),
                                       hipMemcpyDeviceToHost));
        return LK_OK;
    }

  private:
    struct Buf {
        void *slot;                    // the caller's device-pointer variable, set through set()
        void (*set)(void *slot, void *dev);
        const void *src;               // in: host source
        void *dst;                     // out: host destination
        size_t elem, n_dev, n_copy;
        const int64_t *n_back;
        void *dev;
    };
    template <class T> static void set_ptr(void *slot, void *dev) { *static_cast<T **>(slot) = static_cast<T *>(dev); }
    template <class T> StagedCall &none(T *&dev) {
        dev = nullptr;
        return *this;
    }
    template <class T>
    StagedCall &add(T *&dev, const void *src, void *dst, size_t n_dev, size_t n_copy, const int64_t *n_back) {
        dev = nullptr;
        bufs_.push_back({&dev, set_ptr<T>, src, dst, sizeof(T), n_dev, n_copy, n_back, nullptr});
        return *this;
    }
    lk_handle *h_;
    std::vector<Buf> bufs_;
};

}  // namespace lk

using lk::set_error;

extern "C" {

int lk_version(void) { return 101; }

const char *lk_last_error(void) { return lk::g_err.c_str(); }

int lk_device_count(int *count) {
    LK_REQUIRE(count != nullptr, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return LK_EHIP;
    }
    *count = n;
    return LK_OK;
}

int lk_init(int device_id, lk_handle **out) {
    LK_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    int n = 0;
    LK_HIP_CHECK(hipGetDeviceCount(&n));
    LK_REQUIRE(device_id >= 0 && device_id < n, "device_id %d out of range (have %d devices)", device_id, n);
    LK_HIP_CHECK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    LK_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
    lk_handle *h = new (std::nothrow) lk_handle();
    if (!h) return LK_ENOMEM;
    h->device = device_id;
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // the library's ONE environment knob, read once per handle: the chunk size of the pinned host pipeline
    // (lk_set_host_chunk_mb changes it afterwards)
    if (const char *e = getenv("LK_HOST_CHUNK_MB")) h->host_chunk_mb = std::max(1, atoi(e));
    *out = h;
    return LK_OK;
}

int lk_set_host_chunk_mb(lk_handle *h, int mb) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(mb >= 1, "chunk size must be >= 1 MiB");
    h->host_chunk_mb = mb;
    return LK_OK;
}

int lk_bls_set_ordered_histogram(lk_handle *h, int on) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    h->bls_force_serial_hist = on ? 1 : 0;
    return LK_OK;
}

int lk_pld_set_eig_tolerance(lk_handle *h, double tol) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(tol >= 0.0 && tol < 1.0, "tolerance must be in [0, 1) (0 = the default)");
    h->pld_eig_tol = tol;
    return LK_OK;
}

void lk_destroy(lk_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    h->stage.release();
    for (hipStream_t st : {h->s_in, h->s_comp, h->s_out})
        if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t *arr : {h->ev_in, h->ev_comp, h->ev_out})
        for (int i = 0; i < 2; ++i)
            if (arr[i]) (void)hipEventDestroy(arr[i]);
    if (h->h_plan) (void)hipHostFree(h->h_plan);
    if (h->s_probe) (void)hipStreamDestroy(h->s_probe);
    for (int a = 0; a < 3; ++a) {
        if (h->s_ls_aux[a]) (void)hipStreamDestroy(h->s_ls_aux[a]);
        if (h->ev_ls_join[a]) (void)hipEventDestroy(h->ev_ls_join[a]);
    }
    if (h->ev_ls_fork) (void)hipEventDestroy(h->ev_ls_fork);
    if (h->clk_buf) (void)hipHostFree(h->clk_buf);
    if (h->flat_tab_dev) (void)hipFree(h->flat_tab_dev);
    if (h->ls_roots) (void)hipFree(h->ls_roots);
    h->ws.release();
    h->staging.release();
    delete h;
}

int lk_synchronize(lk_handle *h) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    LK_HIP_CHECK(hipDeviceSynchronize());
    return LK_OK;
}

int64_t lk_workspace_bytes(const lk_handle *h) { return h ? (int64_t)(h->ws.cap + h->staging.cap) : 0; }

// ------------------------------------------------------------------------------------------------ LS
int lk_ls_chi2_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                         const double *dy, const double *freq, double f0, double df, int64_t M, int nterms,
                         int fit_mean, int center_data, int normalization, const double *scale, double *power,
                         void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::ls_chi2_launch(h, B, n_off_host, t, y, dy, freq, f0, df, M, nterms, fit_mean, center_data,
                              normalization, scale, power, static_cast<hipStream_t>(stream));
}

int lk_ls_power_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                          const double *dy, const double *freq, double f0, double df, int64_t M, int fit_mean,
                          int center_data, int normalization, const double *scale, double *power, void *stream) {
    return lk_ls_chi2_batch_dev(h, B, n_off_host, t, y, dy, freq, f0, df, M, 1, fit_mean, center_data, normalization,
                                scale, power, stream);
}

int lk_ls_chi2_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y, const double *dy,
                     const double *freq, double f0, double df, int64_t M, int nterms, int fit_mean, int center_data,
                     int normalization, const double *scale, double *power) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    LK_REQUIRE(M >= 0, "M must be >= 0");
    if (B == 0 || M == 0) return LK_OK;
    LK_REQUIRE(t && y && power, "t, y, power must be non-NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *dyv, *ddy, *dfreq, *dscale;
    double *dpow;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(dyv, y, ntot).in(ddy, dy, ntot).in(dfreq, freq, (size_t)M).in(dscale, scale, (size_t)B)
                 .out(dpow, power, (size_t)B * (size_t)M).stage();
    if (rc) return rc;
    rc = lk::ls_chi2_launch(h, B, n_off, dt, dyv, ddy, dfreq, f0, df, M, nterms, fit_mean, center_data, normalization,
                            dscale, dpow, nullptr);
    return rc ? rc : io.finish();
}

int lk_ls_power_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y, const double *dy,
                      const double *freq, double f0, double df, int64_t M, int fit_mean, int center_data,
                      int normalization, const double *scale, double *power) {
    return lk_ls_chi2_batch(h, B, n_off, t, y, dy, freq, f0, df, M, 1, fit_mean, center_data, normalization, scale,
                            power);
}

// ------------------------------------------------------------------------------------------------ fold
int lk_fold_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *period,
                      const double *epoch_time, double epoch_phase, const double *wrap_phase, int normalize_phase,
                      int ncols, const double *const *cols_in, double *const *cols_out, double *phase, int64_t *order,
                      void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fold_launch(h, B, n_off_host, t, period, epoch_time, epoch_phase, wrap_phase, normalize_phase, ncols,
                           cols_in, cols_out, phase, order, static_cast<hipStream_t>(stream));
}

int lk_fold_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *period,
                  const double *epoch_time, double epoch_phase, const double *wrap_phase, int normalize_phase,
                  int ncols, const double *const *cols_in, double *const *cols_out, double *phase, int64_t *order) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && phase && order, "NULL buffer");
    LK_REQUIRE(ncols >= 0 && ncols <= 16 && (ncols == 0 || (cols_in && cols_out)), "bad column list (at most 16 columns)");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *din[16];
    double *dph, *dout[16];
    int64_t *dord;
    lk::StagedCall io(h);
    io.in(dt, t, ntot).out(dph, phase, ntot).out(dord, order, ntot);
    for (int c = 0; c < ncols; ++c) {
        LK_REQUIRE(cols_in[c] && cols_out[c], "column %d is NULL", c);
        io.in(din[c], cols_in[c], ntot).out(dout[c], cols_out[c], ntot);
    }
    int rc = io.stage();
    if (rc) return rc;
    rc = lk::fold_launch(h, B, n_off, dt, period, epoch_time, epoch_phase, wrap_phase, normalize_phase, ncols, din, dout,
                         dph, dord, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ Periodogram.smooth
int lk_pg_logmedian_batch_dev(lk_handle *h, int B, int64_t M, const double *power, int K, const int32_t *win_lo,
                              const int32_t *win_hi, const int32_t *klo, const int32_t *khi, double corr, double *out,
                              void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pg_logmedian_launch(h, B, M, power, K, win_lo, win_hi, klo, khi, corr, out,
                                   static_cast<hipStream_t>(stream));
}

int lk_pg_boxsmooth_batch_dev(lk_handle *h, int B, int64_t M, const double *power, const double *taps, int nk,
                              double *out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pg_boxsmooth_launch(h, B, M, power, taps, nk, out, static_cast<hipStream_t>(stream));
}

int lk_pg_logmedian_batch(lk_handle *h, int B, int64_t M, const double *power, int K, const int32_t *win_lo,
                          const int32_t *win_hi, const int32_t *klo, const int32_t *khi, double corr, double *out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && M >= 1, "need B >= 0 and M >= 1");
    if (B == 0) return LK_OK;
    LK_REQUIRE(power && out, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t n = (size_t)B * (size_t)M;
    const double *dp;
    double *dout;
    lk::StagedCall io(h);
    int rc = io.in(dp, power, n).out(dout, out, n).stage();
    if (rc) return rc;
    rc = lk::pg_logmedian_launch(h, B, M, dp, K, win_lo, win_hi, klo, khi, corr, dout, nullptr);
    return rc ? rc : io.finish();
}

int lk_pg_boxsmooth_batch(lk_handle *h, int B, int64_t M, const double *power, const double *taps, int nk,
                          double *out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && M >= 1, "need B >= 0 and M >= 1");
    if (B == 0) return LK_OK;
    LK_REQUIRE(power && out, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t n = (size_t)B * (size_t)M;
    const double *dp;
    double *dout;
    lk::StagedCall io(h);
    int rc = io.in(dp, power, n).out(dout, out, n).stage();
    if (rc) return rc;
    rc = lk::pg_boxsmooth_launch(h, B, M, dp, taps, nk, dout, nullptr);
    return rc ? rc : io.finish();
}

int lk_pg_acf2d_batch_dev(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int32_t *win_start,
                          int W, double *acf2d, double *metric, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pg_acf2d_launch(h, B, M, power, n_win, win_start, W, acf2d, metric, static_cast<hipStream_t>(stream));
}

int lk_pg_acf2d_batch(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int32_t *win_start, int W,
                      double *acf2d, double *metric) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && M >= 1 && n_win >= 0 && W >= 1, "bad shapes");
    if (B == 0 || n_win == 0) return LK_OK;
    LK_REQUIRE(power && acf2d && metric, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t nm = (size_t)B * n_win;
    const double *dp;
    double *da, *dm;
    lk::StagedCall io(h);
    int rc = io.in(dp, power, (size_t)B * (size_t)M).out(da, acf2d, nm * (size_t)W).out(dm, metric, nm).stage();
    if (rc) return rc;
    rc = lk::pg_acf2d_launch(h, B, M, dp, n_win, win_start, W, da, dm, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ resident seismology
int lk_pg_snr_batch_dev(lk_handle *h, int B, int64_t M, const double *power, const double *bkg, double *out,
                        void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pg_snr_launch(h, B, M, power, bkg, out, static_cast<hipStream_t>(stream));
}

int lk_pg_acf_metric_batch_dev(lk_handle *h, int B, int64_t M, const double *power, int n_win, const int32_t *win_start,
                               int W, double *metric, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pg_acf_metric_launch(h, B, M, power, n_win, win_start, W, metric, static_cast<hipStream_t>(stream));
}

int lk_pg_numax_pick_batch_dev(lk_handle *h, int B, int n_win, const double *metric, const double *taps, int n_taps,
                               double *metric_smooth, int64_t *argmax_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pg_numax_pick_launch(h, B, n_win, metric, taps, n_taps, metric_smooth, argmax_out,
                                    static_cast<hipStream_t>(stream));
}

int lk_pg_deltanu_batch_dev(lk_handle *h, int B, int64_t M, const double *power, const int32_t *start,
                            const int32_t *width, const double *deltanu_emp, const double *distance, const double *step,
                            const double *stop, int max_sel, double *deltanu, int32_t *n_peaks, int32_t *status,
                            int32_t *sel_lo, int32_t *sel_len, double *acf, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pg_deltanu_launch(h, B, M, power, start, width, deltanu_emp, distance, step, stop, max_sel, deltanu,
                                 n_peaks, status, sel_lo, sel_len, acf, static_cast<hipStream_t>(stream));
}

int lk_pg_deltanu_batch(lk_handle *h, int B, int64_t M, const double *power, const int32_t *start, const int32_t *width,
                        const double *deltanu_emp, const double *distance, const double *step, const double *stop,
                        int max_sel, double *deltanu, int32_t *n_peaks, int32_t *status, int32_t *sel_lo,
                        int32_t *sel_len, double *acf) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && M >= 1 && max_sel >= 0, "need B >= 0, M >= 1, max_sel >= 0");
    if (B == 0) return LK_OK;
    LK_REQUIRE(power && deltanu && n_peaks && status && sel_lo && sel_len, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const double *dp;
    double *dd, *da;
    int32_t *dn, *ds, *dlo, *dlen;
    lk::StagedCall io(h);
    int rc = io.in(dp, power, (size_t)B * (size_t)M).out(dd, deltanu, (size_t)B).out(dn, n_peaks, (size_t)B)
                 .out(ds, status, (size_t)B).out(dlo, sel_lo, (size_t)B).out(dlen, sel_len, (size_t)B)
                 .out(da, acf, (size_t)B * (size_t)max_sel).stage();
    if (rc) return rc;
    rc = lk::pg_deltanu_launch(h, B, M, dp, start, width, deltanu_emp, distance, step, stop, max_sel, dd, dn, ds, dlo,
                               dlen, da, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ LS 'fast'
int lk_ls_fast_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                         const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                         int normalization, const double *scale, int oversampling, double *power, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::lsfast_launch(h, B, n_off_host, t, y, dy, f0, df, M, fit_mean, center_data, normalization, scale,
                             oversampling, power, static_cast<hipStream_t>(stream));
}

int lk_ls_fastchi2_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                             const double *dy, double f0, double df, int64_t M, int nterms, int fit_mean,
                             int center_data, int normalization, const double *scale, int oversampling, double *power,
                             void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::lsfastchi2_launch(h, B, n_off_host, t, y, dy, f0, df, M, nterms, fit_mean, center_data, normalization,
                                 scale, oversampling, power, static_cast<hipStream_t>(stream));
}

int lk_ls_fastchi2_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y, const double *dy,
                         double f0, double df, int64_t M, int nterms, int fit_mean, int center_data, int normalization,
                         const double *scale, int oversampling, double *power) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    LK_REQUIRE(M >= 0, "M must be >= 0");
    if (B == 0 || M == 0) return LK_OK;
    LK_REQUIRE(t && y && power, "t, y, power must be non-NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *dyv, *ddy, *dscale;
    double *dpow;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(dyv, y, ntot).in(ddy, dy, ntot).in(dscale, scale, (size_t)B)
                 .out(dpow, power, (size_t)B * (size_t)M).stage();
    if (rc) return rc;
    rc = lk::lsfastchi2_launch(h, B, n_off, dt, dyv, ddy, f0, df, M, nterms, fit_mean, center_data, normalization, dscale,
                               oversampling, dpow, nullptr);
    return rc ? rc : io.finish();
}

int lk_ls_fast_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y, const double *dy,
                     double f0, double df, int64_t M, int fit_mean, int center_data, int normalization,
                     const double *scale, int oversampling, double *power) {
    // chunked, double-buffered staging (lk_ls_fast_peaks_batch below); the multi-term path keeps the simple one
    return lk_ls_fast_peaks_batch(h, B, n_off, t, y, dy, f0, df, M, fit_mean, center_data, normalization, scale,
                                  oversampling, power, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------ argmax
int lk_argmax_batch_dev(lk_handle *h, int B, int64_t M, const double *x, double *max_out, int64_t *argmax_out,
                        void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::argmax_launch(h, B, M, x, max_out, argmax_out, static_cast<hipStream_t>(stream));
}

int lk_argmax_batch(lk_handle *h, int B, int64_t M, const double *x, double *max_out, int64_t *argmax_out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && M >= 1, "need B >= 0 and M >= 1");
    if (B == 0) return LK_OK;
    LK_REQUIRE(x && max_out && argmax_out, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const double *dx;
    double *dm;
    int64_t *da;
    lk::StagedCall io(h);
    int rc = io.in(dx, x, (size_t)B * (size_t)M).out(dm, max_out, (size_t)B).out(da, argmax_out, (size_t)B).stage();
    if (rc) return rc;
    rc = lk::argmax_launch(h, B, M, dx, dm, da, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ BLS
int lk_bls_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                     const double *ivar, const double *period_host, const double *period_dev, int64_t nP,
                     const double *duration_host, int nD, int oversample, int use_likelihood, double *out7,
                     void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::bls_launch(h, B, n_off_host, t, y, ivar, period_host, period_dev, nP, duration_host, nD, oversample,
                          use_likelihood, out7, static_cast<hipStream_t>(stream));
}

int lk_bls_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y, const double *ivar,
                 const double *period, int64_t nP, const double *duration, int nD, int oversample,
                 int use_likelihood, double *out7) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    LK_REQUIRE(nP >= 0 && nD >= 1, "need nP >= 0 and nD >= 1");
    if (B == 0 || nP == 0) return LK_OK;
    LK_REQUIRE(t && y && ivar && period && duration && out7, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *dyv, *div, *dper;
    double *dout;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(dyv, y, ntot).in(div, ivar, ntot).in(dper, period, (size_t)nP)
                 .out(dout, out7, 7 * (size_t)B * (size_t)nP).stage();
    if (rc) return rc;
    rc = lk::bls_launch(h, B, n_off, dt, dyv, div, period, dper, nP, duration, nD, oversample, use_likelihood, dout,
                        nullptr);
    return rc ? rc : io.finish();
}

int lk_bls_max_period(const double *duration, int nD, int oversample, double *max_period) {
    return lk::bls_max_period_host(duration, nD, oversample, max_period);
}

// ------------------------------------------------------------------------------------------------ regression
int lk_regress_cov_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *X, const double *y,
                             const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                             const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                             uint8_t *outlier, double *w_cov, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::regress_launch(h, B, n_off_host, K, X, y, err, cadence_mask, prior_mu, prior_sigma, clip_sigma,
                              niters, w, model, outlier, static_cast<hipStream_t>(stream), w_cov);
}

int lk_regress_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *X, const double *y,
                         const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                         const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                         uint8_t *outlier, void *stream) {
    return lk_regress_cov_batch_dev(h, B, n_off_host, K, X, y, err, cadence_mask, prior_mu, prior_sigma, clip_sigma,
                                    niters, w, model, outlier, nullptr, stream);
}

int lk_regress_batch(lk_handle *h, int B, const int64_t *n_off, int K, const double *X, const double *y,
                     const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                     const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                     uint8_t *outlier) {
    return lk_regress_cov_batch(h, B, n_off, K, X, y, err, cadence_mask, prior_mu, prior_sigma, clip_sigma, niters, w,
                                model, outlier, nullptr);
}

int lk_regress_cov_batch(lk_handle *h, int B, const int64_t *n_off, int K, const double *X, const double *y,
                         const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                         const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                         uint8_t *outlier, double *w_cov) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(K >= 1, "K must be >= 1");
    LK_REQUIRE(X && y && w && model && outlier, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], nk = (size_t)B * K;
    const double *dX, *dy, *derr, *dmu, *dsg;
    const uint8_t *dcm;
    double *dmodel, *dw, *dcov;
    uint8_t *dout;
    lk::StagedCall io(h);
    int rc = io.in(dX, X, ntot * (size_t)K).in(dy, y, ntot).in(derr, err, ntot).out(dmodel, model, ntot)
                 .in(dcm, cadence_mask, ntot).out(dout, outlier, ntot).in(dmu, prior_mu, nk).in(dsg, prior_sigma, nk)
                 .out(dw, w, nk).out(dcov, w_cov, nk * K).stage();
    if (rc) return rc;
    rc = lk::regress_launch(h, B, n_off, K, dX, dy, derr, dcm, dmu, dsg, clip_sigma, niters, dw, dmodel, dout,
                            nullptr, dcov);
    return rc ? rc : io.finish();
}

// one design matrix shared by all targets
int lk_regress_shared_batch_dev(lk_handle *h, int B, int N, int K, const double *X, const double *y, const double *err,
                                const uint8_t *cadence_mask, const double *prior_mu, const double *prior_sigma,
                                double clip_sigma, int niters, double *w, double *model, uint8_t *outlier, double *w_cov,
                                void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::regress_shared_launch(h, B, N, K, X, y, err, cadence_mask, prior_mu, prior_sigma, clip_sigma, niters, w, model,
                                     outlier, w_cov, static_cast<hipStream_t>(stream));
}

int lk_regress_shared_batch(lk_handle *h, int B, int N, int K, const double *X, const double *y, const double *err,
                            const uint8_t *cadence_mask, const double *prior_mu, const double *prior_sigma,
                            double clip_sigma, int niters, double *w, double *model, uint8_t *outlier, double *w_cov) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(K >= 1 && N >= 1, "K and N must be >= 1");
    LK_REQUIRE(X && y && w && model && outlier, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)B * N, nk = (size_t)B * K;
    const double *dX, *dy, *derr, *dmu, *dsg;
    const uint8_t *dcm;
    double *dmodel, *dw, *dcov;
    uint8_t *dout;
    lk::StagedCall io(h);
    int rc = io.in(dX, X, (size_t)N * K).in(dy, y, ntot).in(derr, err, ntot).out(dmodel, model, ntot)
                 .in(dcm, cadence_mask, ntot).out(dout, outlier, ntot).in(dmu, prior_mu, nk).in(dsg, prior_sigma, nk)
                 .out(dw, w, nk).out(dcov, w_cov, nk * K).stage();
    if (rc) return rc;
    rc = lk::regress_shared_launch(h, B, N, K, dX, dy, derr, dcm, dmu, dsg, clip_sigma, niters, dw, dmodel, dout, dcov, nullptr);
    return rc ? rc : io.finish();
}

int lk_ridge_prior_batch_dev(lk_handle *h, int B, int N, int K, const double *flux_err, double alpha, double *prior_mu,
                             double *prior_sigma, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::ridge_prior_launch(h, B, N, K, flux_err, alpha, nullptr, prior_mu, prior_sigma, static_cast<hipStream_t>(stream));
}

int lk_ridge_prior_alphas_batch_dev(lk_handle *h, int B, int N, int K, const double *flux_err, const double *alpha,
                                    double *prior_mu, double *prior_sigma, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(alpha != nullptr, "alpha is NULL (B doubles on the device)");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::ridge_prior_launch(h, B, N, K, flux_err, 0.0, alpha, prior_mu, prior_sigma, static_cast<hipStream_t>(stream));
}

// one design matrix, ragged targets aligned by cadence number
int lk_align_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *cadenceno, int Nx,
                            const int32_t *grid_cadenceno, int32_t *rows, int32_t *pos, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::align_rows_launch(h, B, n_off_host, cadenceno, Nx, grid_cadenceno, rows, pos, static_cast<hipStream_t>(stream));
}

int lk_align_rows_batch(lk_handle *h, int B, const int64_t *n_off, const int32_t *cadenceno, int Nx, const int32_t *grid_cadenceno,
                        int32_t *rows, int32_t *pos) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(Nx >= 1 && n_off[B] >= 0, "bad shapes");
    LK_REQUIRE(cadenceno && grid_cadenceno && rows, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const int32_t *dc, *dg;
    int32_t *dr, *dp;
    lk::StagedCall io(h);
    int rc = io.in(dc, cadenceno, ntot).in(dg, grid_cadenceno, (size_t)Nx).out(dr, rows, ntot).out(dp, pos, (size_t)B * Nx).stage();
    if (rc) return rc;
    rc = lk::align_rows_launch(h, B, n_off, dc, Nx, dg, dr, dp, nullptr);
    return rc ? rc : io.finish();
}

int lk_regress_shared_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx, int K,
                                     const double *X, const double *y, const double *err, const uint8_t *cadence_mask,
                                     const double *prior_mu, const double *prior_sigma, double clip_sigma, int niters, double *w,
                                     double *model, uint8_t *outlier, double *w_cov, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::regress_shared_rows_launch(h, B, n_off_host, rows, Nx, K, X, y, err, cadence_mask, prior_mu, prior_sigma, clip_sigma,
                                          niters, w, model, outlier, w_cov, static_cast<hipStream_t>(stream));
}

int lk_regress_shared_rows_batch(lk_handle *h, int B, const int64_t *n_off, const int32_t *rows, int Nx, int K, const double *X,
                                 const double *y, const double *err, const uint8_t *cadence_mask, const double *prior_mu,
                                 const double *prior_sigma, double clip_sigma, int niters, double *w, double *model,
                                 uint8_t *outlier, double *w_cov) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(K >= 1 && Nx >= 1 && n_off[B] >= 0, "K and Nx must be >= 1");
    LK_REQUIRE(rows && X && y && w && model && outlier, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], nk = (size_t)B * K;
    const int32_t *drows;
    const double *dX, *dy, *derr, *dmu, *dsg;
    const uint8_t *dcm;
    double *dmodel, *dw, *dcov;
    uint8_t *dout;
    lk::StagedCall io(h);
    int rc = io.in(drows, rows, ntot).in(dX, X, (size_t)Nx * K).in(dy, y, ntot).in(derr, err, ntot).out(dmodel, model, ntot)
                 .in(dcm, cadence_mask, ntot).out(dout, outlier, ntot).in(dmu, prior_mu, nk).in(dsg, prior_sigma, nk)
                 .out(dw, w, nk).out(dcov, w_cov, nk * K).stage();
    if (rc) return rc;
    rc = lk::regress_shared_rows_launch(h, B, n_off, drows, Nx, K, dX, dy, derr, dcm, dmu, dsg, clip_sigma, niters, dw, dmodel, dout,
                                        dcov, nullptr);
    return rc ? rc : io.finish();
}

int lk_ridge_prior_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *flux_err, double alpha,
                                  double *prior_mu, double *prior_sigma, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::ridge_prior_rows_launch(h, B, n_off_host, K, flux_err, alpha, nullptr, prior_mu, prior_sigma,
                                       static_cast<hipStream_t>(stream));
}

int lk_ridge_prior_rows_alphas_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, int K, const double *flux_err,
                                         const double *alpha, double *prior_mu, double *prior_sigma, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(alpha != nullptr, "alpha is NULL (B doubles on the device)");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::ridge_prior_rows_launch(h, B, n_off_host, K, flux_err, 0.0, alpha, prior_mu, prior_sigma,
                                       static_cast<hipStream_t>(stream));
}

// host pointers; alphas nullable (then `alpha` for every target)
static int ridge_prior_rows_host(lk_handle *h, int B, const int64_t *n_off, int K, const double *flux_err, double alpha,
                                 const double *alphas, double *prior_mu, double *prior_sigma) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && K >= 1 && n_off != nullptr && n_off[B] >= 0, "bad shapes");
    LK_REQUIRE(flux_err && prior_mu && prior_sigma, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t nk = (size_t)B * K;
    const double *de, *da;
    double *dmu, *dsg;
    lk::StagedCall io(h);
    int rc = io.in(de, flux_err, (size_t)n_off[B]).in(da, alphas, (size_t)B).out(dmu, prior_mu, nk).out(dsg, prior_sigma, nk).stage();
    if (rc) return rc;
    rc = lk::ridge_prior_rows_launch(h, B, n_off, K, de, alpha, da, dmu, dsg, nullptr);
    return rc ? rc : io.finish();
}

int lk_ridge_prior_rows_batch(lk_handle *h, int B, const int64_t *n_off, int K, const double *flux_err, double alpha,
                              double *prior_mu, double *prior_sigma) {
    return ridge_prior_rows_host(h, B, n_off, K, flux_err, alpha, nullptr, prior_mu, prior_sigma);
}

int lk_ridge_prior_rows_alphas_batch(lk_handle *h, int B, const int64_t *n_off, int K, const double *flux_err, const double *alpha,
                                     double *prior_mu, double *prior_sigma) {
    LK_REQUIRE(alpha != nullptr, "alpha is NULL (B doubles)");
    return ridge_prior_rows_host(h, B, n_off, K, flux_err, 0.0, alpha, prior_mu, prior_sigma);
}

// shared columns on knots -> per-target design matrices by PCHIP (interp.hip)
int lk_pchip_interp_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, int Nx, int K,
                              const double *knot_time, const double *Y, const uint8_t *knot_keep, int extrapolate,
                              int append_constant, double *X_out, uint8_t *inside, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pchip_interp_launch(h, B, n_off_host, t, Nx, K, knot_time, Y, knot_keep, extrapolate, append_constant, X_out, inside,
                                   static_cast<hipStream_t>(stream));
}

int lk_pchip_interp_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, int Nx, int K, const double *knot_time,
                          const double *Y, const uint8_t *knot_keep, int extrapolate, int append_constant, double *X_out,
                          uint8_t *inside) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr && n_off[B] >= 0, "bad batch description");
    LK_REQUIRE(K >= 1 && Nx >= 2, "K must be >= 1 and Nx >= 2");
    LK_REQUIRE(knot_time && Y && (n_off[B] == 0 || (t && (X_out || inside))), "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], kout = (size_t)K + (append_constant ? 1 : 0);
    const double *dt, *dx, *dY;
    const uint8_t *dkeep;
    double *dX;
    uint8_t *din;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(dx, knot_time, (size_t)Nx).in(dY, Y, (size_t)Nx * K).in(dkeep, knot_keep, (size_t)Nx)
                 .out(dX, X_out, ntot * kout).out(din, inside, ntot).stage();
    if (rc) return rc;
    rc = lk::pchip_interp_launch(h, B, n_off, dt, Nx, K, dx, dY, dkeep, extrapolate, append_constant, dX, din, nullptr);
    return rc ? rc : io.finish();
}

int lk_subtract_f64_dev(lk_handle *h, int64_t n, const double *a, const double *b, double *out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::subtract_launch(h, n, a, b, out, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ under-fitting metric
int lk_underfit_neighbors_batch_dev(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int M,
                                    const int32_t *neighbors, double *corr, double *metric, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::underfit_neighbors_launch(h, B, N, flux, n, keep_idx, M, neighbors, corr, metric, static_cast<hipStream_t>(stream));
}

int lk_underfit_neighbors_batch(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int M,
                                const int32_t *neighbors, double *corr, double *metric) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1, "B must be >= 1 (got %d)", B);
    LK_REQUIRE(N >= 2 && n >= 2 && n <= N, "need 2 <= n <= N (got n=%d, N=%d): the metric needs at least two kept cadences", n, N);
    LK_REQUIRE(keep_idx != nullptr || n == N, "keep_idx is NULL (all cadences) but n=%d != N=%d", n, N);
    LK_REQUIRE(M >= 0, "M must be >= 0 (got %d)", M);
    LK_REQUIRE(flux && metric, "NULL buffer");
    LK_REQUIRE(M == 0 || neighbors != nullptr, "neighbors is NULL with M=%d", M);
    if (keep_idx)
        for (int i = 0; i < n; ++i)
            LK_REQUIRE(keep_idx[i] >= 0 && keep_idx[i] < N && (i == 0 || keep_idx[i] > keep_idx[i - 1]),
                       "keep_idx[%d]=%d: the kept cadences must be ascending indices in [0, %d)", i, keep_idx[i], N);
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < M; ++p) {
            const int32_t j = neighbors[(size_t)b * M + p];
            LK_REQUIRE(j == -1 || (j >= 0 && j < B), "neighbors[%d][%d]=%d: a neighbour is -1 (padding) or an index in [0, %d)", b, p,
                       (int)j, B);
            LK_REQUIRE(j != b, "neighbors[%d][%d]=%d: a target cannot be its own neighbour", b, p, (int)j);
        }
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t nm = (size_t)B * M;
    const double *dflux;
    const int32_t *dkeep, *dnbr;
    double *dcorr, *dmetric;
    lk::StagedCall io(h);
    int rc = io.in(dflux, flux, (size_t)B * N).in(dkeep, keep_idx, (size_t)n).in(dnbr, M ? neighbors : nullptr, nm)
                 .out(dcorr, M ? corr : nullptr, nm).out(dmetric, metric, (size_t)B).stage();
    if (rc) return rc;
    rc = lk::underfit_neighbors_launch(h, B, N, dflux, n, dkeep, M, dnbr, dcorr, dmetric, nullptr);
    return rc ? rc : io.finish();
}

int lk_underfit_rows_bytes(int Bn, int n, int64_t *bytes) { return lk::underfit_rows_bytes(Bn, n, bytes); }

int lk_underfit_rows_prepare_dev(lk_handle *h, int Bn, int N, const double *flux_nb, int n, const int32_t *keep_idx, void *rows,
                                 int64_t rows_bytes, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::underfit_rows_prepare_launch(h, Bn, N, flux_nb, n, keep_idx, rows, rows_bytes, static_cast<hipStream_t>(stream));
}

int lk_underfit_against_rows_batch_dev(lk_handle *h, int B, int N, const double *flux, int n, const int32_t *keep_idx, int Bn,
                                       const void *rows, int M, const int32_t *neighbors, double *corr, double *metric,
                                       void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::underfit_against_rows_launch(h, B, N, flux, n, keep_idx, Bn, rows, M, neighbors, corr, metric,
                                            static_cast<hipStream_t>(stream));
}

// ragged targets on a cadence grid
int lk_underfit_grid_neighbors_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx,
                                         const double *flux, const uint8_t *cadence_mask, int M, const int32_t *neighbors,
                                         double *corr, int32_t *n_common, double *metric, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::underfit_grid_neighbors_launch(h, B, n_off_host, rows, Nx, flux, cadence_mask, M, neighbors, corr, n_common, metric,
                                              static_cast<hipStream_t>(stream));
}

int lk_underfit_grid_neighbors_batch(lk_handle *h, int B, const int64_t *n_off, const int32_t *rows, int Nx, const double *flux,
                                     const uint8_t *cadence_mask, int M, const int32_t *neighbors, double *corr, int32_t *n_common,
                                     double *metric) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && n_off != nullptr, "B must be >= 1 (got %d) and n_off given", B);
    LK_REQUIRE(Nx >= 1 && n_off[0] == 0 && n_off[B] >= 0, "bad shapes");
    LK_REQUIRE(M >= 0, "M must be >= 0 (got %d)", M);
    LK_REQUIRE(rows && flux && metric, "NULL buffer");
    LK_REQUIRE(M == 0 || neighbors != nullptr, "neighbors is NULL with M=%d", M);
    for (int b = 0; b < B; ++b) {
        LK_REQUIRE(n_off[b + 1] >= n_off[b], "n_off must not decrease (target %d)", b);
        for (int64_t i = n_off[b]; i < n_off[b + 1]; ++i)
            LK_REQUIRE(rows[i] >= 0 && rows[i] < Nx && (i == n_off[b] || rows[i] > rows[i - 1]),
                       "target %d: rows must be strictly increasing indices into the %d rows of the grid", b, Nx);
        for (int p = 0; p < M; ++p) {
            const int32_t j = neighbors[(size_t)b * M + p];
            LK_REQUIRE(j == -1 || (j >= 0 && j < B), "neighbors[%d][%d]=%d: a neighbour is -1 (padding) or an index in [0, %d)", b, p,
                       (int)j, B);
            LK_REQUIRE(j != b, "neighbors[%d][%d]=%d: a target cannot be its own neighbour", b, p, (int)j);
        }
    }
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], nm = (size_t)B * M;
    const int32_t *drows, *dnbr;
    const double *dflux;
    const uint8_t *dcm;
    double *dcorr, *dmetric;
    int32_t *dnc;
    lk::StagedCall io(h);
    int rc = io.in(drows, rows, ntot).in(dflux, flux, ntot).in(dcm, cadence_mask, ntot).in(dnbr, M ? neighbors : nullptr, nm)
                 .out(dcorr, M ? corr : nullptr, nm).out(dnc, n_common, (size_t)B).out(dmetric, metric, (size_t)B).stage();
    if (rc) return rc;
    rc = lk::underfit_grid_neighbors_launch(h, B, n_off, drows, Nx, dflux, dcm, M, dnbr, dcorr, dnc, dmetric, nullptr);
    return rc ? rc : io.finish();
}

int lk_underfit_grid_rows_bytes(int Bn, int Nx, int64_t *bytes) { return lk::underfit_grid_rows_bytes(Bn, Nx, bytes); }

int lk_underfit_grid_rows_prepare_dev(lk_handle *h, int Bn, const int64_t *n_off_host, const int32_t *rows, int Nx,
                                      const double *flux_nb, const uint8_t *cadence_mask, void *block, int64_t block_bytes,
                                      void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::underfit_grid_rows_prepare_launch(h, Bn, n_off_host, rows, Nx, flux_nb, cadence_mask, block, block_bytes,
                                                 static_cast<hipStream_t>(stream));
}

int lk_underfit_grid_against_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int32_t *rows, int Nx,
                                            const double *flux, const uint8_t *cadence_mask, int Bn, const void *block, int M,
                                            const int32_t *neighbors, double *corr, int32_t *n_common, double *metric,
                                            void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::underfit_grid_against_rows_launch(h, B, n_off_host, rows, Nx, flux, cadence_mask, Bn, block, M, neighbors, corr,
                                                 n_common, metric, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ over-fitting metric
int lk_overfit_scratch_bytes(int B, int n, int64_t M, int n_samples, int64_t max_scratch_bytes, int64_t *bytes,
                             int *samples_per_round) {
    return lk::overfit_scratch_bytes(B, n, M, n_samples, max_scratch_bytes, bytes, samples_per_round);
}

int lk_overfit_noise_batch_dev(lk_handle *h, int B, int n, int k, uint64_t seed, int64_t first_target, int64_t stream_id,
                               double *out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::overfit_noise_launch(h, B, n, k, seed, first_target, stream_id, out, static_cast<hipStream_t>(stream));
}

int lk_overfit_metric_batch_dev(lk_handle *h, int B, int N, const double *time, const double *flux_orig, const double *flux_corr,
                                const double *err_corr, int n, const int32_t *keep_idx, double f0, double df, int64_t M,
                                int n_samples, uint64_t seed, int64_t first_target, int64_t stream_id, void *scratch,
                                int64_t scratch_bytes, double *metric, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::overfit_metric_launch(h, lk::OverfitBatch::uniform(B, N, n, keep_idx), time, flux_orig, flux_corr, err_corr, f0, df, M,
                                     n_samples, seed, first_target, stream_id, scratch, scratch_bytes, metric,
                                     static_cast<hipStream_t>(stream));
}

int lk_overfit_session_bytes(int B, int n, int64_t M, int n_samples, int64_t max_scratch_bytes, int64_t *bytes,
                             int *samples_per_round) {
    return lk::overfit_scratch_bytes(B, n, M, n_samples, max_scratch_bytes, bytes, samples_per_round);
}

int lk_overfit_session_begin_dev(lk_handle *h, int B, int N, const double *time, const double *flux_orig, int n,
                                 const int32_t *keep_idx, double f0, double df, int64_t M, int n_samples, uint64_t seed,
                                 int64_t first_target, int64_t stream_id, void *session, int64_t session_bytes, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::overfit_session_begin_launch(h, lk::OverfitBatch::uniform(B, N, n, keep_idx), time, flux_orig, f0, df, M, n_samples, seed,
                                            first_target, stream_id, session, session_bytes, static_cast<hipStream_t>(stream));
}

int lk_overfit_session_eval_dev(lk_handle *h, int B, int N, const double *flux_corr, const double *err_corr, int n,
                                const int32_t *keep_idx, double f0, double df, int64_t M, int n_samples, void *session,
                                int64_t session_bytes, double *metric, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::overfit_session_eval_launch(h, lk::OverfitBatch::uniform(B, N, n, keep_idx), flux_corr, err_corr, f0, df, M, n_samples,
                                           session, session_bytes, metric, static_cast<hipStream_t>(stream));
}

int lk_overfit_metric_batch(lk_handle *h, int B, int N, const double *time, const double *flux_orig, const double *flux_corr,
                            const double *err_corr, int n, const int32_t *keep_idx, double f0, double df, int64_t M, int n_samples,
                            uint64_t seed, int64_t first_target, int64_t stream_id, int64_t max_scratch_bytes, double *metric) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(N >= 3 && N < (1 << 30) && n <= N, "need n <= N < 2^30 (got n=%d, N=%d)", n, N);
    LK_REQUIRE(keep_idx != nullptr || n == N, "keep_idx is NULL (all cadences) but n=%d != N=%d", n, N);
    LK_REQUIRE(time && flux_orig && flux_corr && err_corr && metric, "NULL buffer");
    int64_t bytes = 0;
    int rc = lk::overfit_scratch_bytes(B, n, M, n_samples, max_scratch_bytes, &bytes, nullptr);
    if (rc) return rc;
    if (keep_idx)
        for (int i = 0; i < n; ++i)
            LK_REQUIRE(keep_idx[i] >= 0 && keep_idx[i] < N && (i == 0 || keep_idx[i] > keep_idx[i - 1]),
                       "keep_idx[%d]=%d: the kept cadences must be ascending indices in [0, %d)", i, keep_idx[i], N);
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t bn = (size_t)B * N;
    const double *dt, *dy0, *dy1, *de1;
    const int32_t *dkeep;
    double *dmetric;
    char *dscr;
    lk::StagedCall io(h);
    rc = io.in(dt, time, bn).in(dy0, flux_orig, bn).in(dy1, flux_corr, bn).in(de1, err_corr, bn).in(dkeep, keep_idx, (size_t)n)
             .out(dmetric, metric, (size_t)B).scratch(dscr, (size_t)bytes).stage();
    if (rc) return rc;
    rc = lk::overfit_metric_launch(h, lk::OverfitBatch::uniform(B, N, n, dkeep), dt, dy0, dy1, de1, f0, df, M, n_samples, seed, first_target,
                                   stream_id, dscr, bytes, dmetric, nullptr);
    return rc ? rc : io.finish();
}

// the batch's own offsets
int lk_overfit_scratch_rows_bytes(int B, const int64_t *k_off_host, int64_t M, int n_samples, int64_t max_scratch_bytes,
                                  int64_t *bytes, int *samples_per_round) {
    return lk::overfit_scratch_rows_bytes(B, k_off_host, M, n_samples, max_scratch_bytes, bytes, samples_per_round);
}

int lk_overfit_session_rows_bytes(int B, const int64_t *k_off_host, int64_t M, int n_samples, int64_t max_scratch_bytes,
                                  int64_t *bytes, int *samples_per_round) {
    return lk::overfit_scratch_rows_bytes(B, k_off_host, M, n_samples, max_scratch_bytes, bytes, samples_per_round);
}

int lk_overfit_metric_rows_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux_orig,
                                     const double *flux_corr, const double *err_corr, const int32_t *keep_idx,
                                     const int64_t *k_off_host, double f0, double df, int64_t M, int n_samples, uint64_t seed,
                                     int64_t first_target, int64_t stream_id, void *scratch, int64_t scratch_bytes, double *metric,
                                     void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::overfit_metric_launch(h, lk::OverfitBatch::rows(B, n_off_host, keep_idx, k_off_host), time, flux_orig, flux_corr, err_corr, f0,
                                     df, M, n_samples, seed, first_target, stream_id, scratch, scratch_bytes, metric,
                                     static_cast<hipStream_t>(stream));
}

int lk_overfit_session_begin_rows_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux_orig,
                                      const int32_t *keep_idx, const int64_t *k_off_host, double f0, double df, int64_t M,
                                      int n_samples, uint64_t seed, int64_t first_target, int64_t stream_id, void *session,
                                      int64_t session_bytes, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::overfit_session_begin_launch(h, lk::OverfitBatch::rows(B, n_off_host, keep_idx, k_off_host), time, flux_orig, f0, df, M,
                                            n_samples, seed, first_target, stream_id, session, session_bytes,
                                            static_cast<hipStream_t>(stream));
}

int lk_overfit_session_eval_rows_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *flux_corr, const double *err_corr,
                                     const int32_t *keep_idx, const int64_t *k_off_host, double f0, double df, int64_t M,
                                     int n_samples, void *session, int64_t session_bytes, double *metric, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::overfit_session_eval_launch(h, lk::OverfitBatch::rows(B, n_off_host, keep_idx, k_off_host), flux_corr, err_corr, f0, df, M,
                                           n_samples, session, session_bytes, metric, static_cast<hipStream_t>(stream));
}

int lk_overfit_metric_rows_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux_orig,
                                 const double *flux_corr, const double *err_corr, const int32_t *keep_idx, const int64_t *k_off,
                                 double f0, double df, int64_t M, int n_samples, uint64_t seed, int64_t first_target,
                                 int64_t stream_id, int64_t max_scratch_bytes, double *metric) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && n_off != nullptr && n_off[0] == 0, "B must be >= 1 (got %d) and n_off given, starting at 0", B);
    LK_REQUIRE((keep_idx == nullptr) == (k_off == nullptr || k_off == n_off), "keep_idx and k_off go together");
    LK_REQUIRE(time && flux_orig && flux_corr && err_corr && metric, "NULL buffer");
    const int64_t *ko = k_off ? k_off : n_off;
    int64_t bytes = 0;
    int rc = lk::overfit_scratch_rows_bytes(B, ko, M, n_samples, max_scratch_bytes, &bytes, nullptr);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        const int64_t N = n_off[b + 1] - n_off[b];
        LK_REQUIRE(N >= 3 && N < (1 << 30), "target %d: %lld cadences outside 3..2^30", b, (long long)N);
        if (keep_idx)
            for (int64_t i = ko[b]; i < ko[b + 1]; ++i)
                LK_REQUIRE(keep_idx[i] >= 0 && keep_idx[i] < N && (i == ko[b] || keep_idx[i] > keep_idx[i - 1]),
                           "target %d: the kept cadences must be ascending indices in [0, %lld)", b, (long long)N);
    }
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *dy0, *dy1, *de1;
    const int32_t *dkeep;
    double *dmetric;
    char *dscr;
    lk::StagedCall io(h);
    rc = io.in(dt, time, ntot).in(dy0, flux_orig, ntot).in(dy1, flux_corr, ntot).in(de1, err_corr, ntot)
             .in(dkeep, keep_idx, (size_t)ko[B]).out(dmetric, metric, (size_t)B).scratch(dscr, (size_t)bytes).stage();
    if (rc) return rc;
    rc = lk::overfit_metric_launch(h, lk::OverfitBatch::rows(B, n_off, dkeep, keep_idx ? ko : nullptr), dt, dy0, dy1, de1, f0, df, M,
                                   n_samples, seed, first_target, stream_id, dscr, bytes, dmetric, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ flatten
int lk_savgol_design(int window, int polyorder, double *coeffs, double *edge) {
    return lk::savgol_design_host(window, polyorder, coeffs, edge);
}

int lk_savgol_trend_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                              const uint8_t *mask, int window, int polyorder, double break_tol, int niters,
                              double sigma, double *trend, uint8_t *fit_mask, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::flatten_launch(h, B, n_off_host, t, flux, mask, window, polyorder, break_tol, niters, sigma, trend,
                              fit_mask, static_cast<hipStream_t>(stream));
}

int lk_savgol_trend_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux,
                          const uint8_t *mask, int window, int polyorder, double break_tol, int niters, double sigma,
                          double *trend, uint8_t *fit_mask) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && flux && trend, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *df;
    const uint8_t *dm;
    double *dtr;
    uint8_t *dfm;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(df, flux, ntot).out(dtr, trend, ntot).in(dm, mask, ntot).out(dfm, fit_mask, ntot)
                 .stage();
    if (rc) return rc;
    rc = lk::flatten_launch(h, B, n_off, dt, df, dm, window, polyorder, break_tol, niters, sigma, dtr, dfm, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ PLD design matrix
int lk_pld_design_width(int P, int Pb, int pld_order, int pca_components, int n_knots) {
    return lk::pld_design_width(P, Pb, pld_order, pca_components, n_knots);
}

int lk_pld_design_batch_dev(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                            const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                            int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, double *X,
                            double *prior_sigma, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pld_design_launch(h, B, N, P, Pb, pld_pix, bkg_pix, lc_flux, time, knots, n_inner, pld_order,
                                 pca_components, n_knots, spline_degree, normalize_bkg, K, X, prior_sigma,
                                 static_cast<hipStream_t>(stream));
}

int lk_pld_design_batch(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                        const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                        int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, double *X,
                        double *prior_sigma) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && N >= 2 && P >= 0 && Pb >= 1 && K >= 1, "bad shapes");
    LK_REQUIRE(bkg_pix && lc_flux && time && knots && X && prior_sigma, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t bn = (size_t)B * N;
    const float *dp, *db, *dl;
    const double *dt, *dk;
    double *dX, *ds;
    lk::StagedCall io(h);
    int rc = io.in(dp, P > 0 ? pld_pix : nullptr, bn * P).in(db, bkg_pix, bn * Pb).in(dl, lc_flux, bn).in(dt, time, bn)
                 .in(dk, knots, (size_t)B * (n_inner + 2)).out(dX, X, bn * K).out(ds, prior_sigma, (size_t)B * K).stage();
    if (rc) return rc;
    rc = lk::pld_design_launch(h, B, N, dp ? P : 0, Pb, dp, db, dl, dt, dk, n_inner, pld_order, pca_components, n_knots,
                               spline_degree, normalize_bkg, K, dX, ds, nullptr);
    return rc ? rc : io.finish();
}

// PLDCorrector.correct for B same-shaped cutouts, host pointers in and out: design matrices, regression + clip loop and the
// spline block's share of the model in one call — X (B x N x K doubles, 1.7 GB per 500 K2 cutouts) never leaves HBM.
// Per-cutout column counts of a ragged call, on the host: each within [pca_components, pitch] (one design width per call).
static int pld_check_counts(const char *what, const int32_t *count, int B, int pitch, int pca_components) {
    for (int b = 0; count && b < B; ++b)
        LK_REQUIRE(count[b] >= pca_components && count[b] >= 1 && count[b] <= pitch,
                   "cutout %d has %d %s pixels: a ragged call needs between pca_components = %d and the row pitch %d in every cutout",
                   b, (int)count[b], what, pca_components, pitch);
    return LK_OK;
}

static int pld_correct_host(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                            const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                            int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, const double *y,
                            const double *err, const uint8_t *cadence_mask, double clip_sigma, int niters, double *w,
                            double *model, uint8_t *outlier, double *spline_part, const int32_t *p_count,
                            const int32_t *pb_count) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && N >= 2 && P >= 0 && Pb >= 1 && K >= 1, "bad shapes");
    LK_REQUIRE(bkg_pix && lc_flux && time && knots && y && w && model && outlier, "NULL buffer");
    LK_REQUIRE(n_knots + 1 <= K, "K=%d is narrower than the spline block (%d columns)", K, n_knots + 1);
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t bn = (size_t)B * N;
    const bool has_pld = P > 0 && pld_pix != nullptr;
    const bool shared = has_pld && pld_pix == bkg_pix && P == Pb;  // one aperture for both blocks: one upload
    const size_t nk = (size_t)B * K;
    const float *dp, *db, *dl;
    const double *dt, *dk, *dy, *derr;
    const uint8_t *dcm;
    const int32_t *dpc, *dbc;
    double *dX, *ds, *dmu, *dw, *dmodel, *dsp;
    uint8_t *dout;
    int rc = pld_check_counts("PLD", has_pld ? p_count : nullptr, B, P, pca_components);
    if (!rc) rc = pld_check_counts("background", pb_count, B, Pb, pca_components);
    if (rc) return rc;
    lk::StagedCall io(h);
    rc = io.in(dp, has_pld && !shared ? pld_pix : nullptr, bn * P).in(db, bkg_pix, bn * Pb).in(dl, lc_flux, bn)
             .in(dt, time, bn).in(dk, knots, (size_t)B * (n_inner + 2)).scratch(dX, bn * K).scratch(ds, nk)
             .scratch(dmu, nk).out(dw, w, nk).in(dy, y, bn).in(derr, err, bn).out(dmodel, model, bn)
             .out(dsp, spline_part, bn).in(dcm, cadence_mask, bn).out(dout, outlier, bn)
             .in(dpc, has_pld ? p_count : nullptr, (size_t)B).in(dbc, pb_count, (size_t)B).stage();
    if (rc) return rc;
    if (shared) dp = db;
    LK_HIP_CHECK(hipMemsetAsync(dmu, 0, nk * 8, nullptr));   // prior_mu = 0 for every PLD column (pldcorrector.py:240-287)
    rc = lk::pld_design_launch(h, B, N, dp ? P : 0, Pb, dp, db, dl, dt, dk, n_inner, pld_order, pca_components, n_knots,
                               spline_degree, normalize_bkg, K, dX, ds, nullptr, dpc, dbc);
    if (rc) return rc;
    std::vector<int64_t> off((size_t)B + 1);
    for (int b = 0; b <= B; ++b) off[b] = (int64_t)b * N;
    rc = lk::regress_launch(h, B, off.data(), K, dX, dy, derr, dcm, dmu, ds, clip_sigma, niters, dw, dmodel, dout, nullptr);
    if (rc) return rc;
    if (dsp) {
        rc = lk::model_part_launch(h, B, N, K, K - (n_knots + 1), K, dX, dw, dsp, nullptr);
        if (rc) return rc;
    }
    return io.finish();
}

int lk_pld_correct_batch(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                         const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                         int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, const double *y,
                         const double *err, const uint8_t *cadence_mask, double clip_sigma, int niters, double *w,
                         double *model, uint8_t *outlier, double *spline_part) {
    return pld_correct_host(h, B, N, P, Pb, pld_pix, bkg_pix, lc_flux, time, knots, n_inner, pld_order, pca_components, n_knots,
                            spline_degree, normalize_bkg, K, y, err, cadence_mask, clip_sigma, niters, w, model, outlier,
                            spline_part, nullptr, nullptr);
}

// lk_pld_correct_batch for cutouts whose pixel blocks hold different numbers of real columns: cutout b's first p_count[b] /
// pb_count[b] columns (host arrays of B entries, NULL = all of them) are pixels, the rest of the row pitch P / Pb is +0.0f.
int lk_pld_correct_ragged_batch(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                                const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                                int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, const double *y,
                                const double *err, const uint8_t *cadence_mask, double clip_sigma, int niters, double *w,
                                double *model, uint8_t *outlier, double *spline_part, const int32_t *p_count,
                                const int32_t *pb_count) {
    return pld_correct_host(h, B, N, P, Pb, pld_pix, bkg_pix, lc_flux, time, knots, n_inner, pld_order, pca_components, n_knots,
                            spline_degree, normalize_bkg, K, y, err, cadence_mask, clip_sigma, niters, w, model, outlier,
                            spline_part, p_count, pb_count);
}

// lk_pld_correct_batch on device pointers and a stream.  X, prior_sigma and prior_mu are the CALLER's device scratch, not
// h->staging: a later host-pointer call on this handle re-carves the staging arena while `stream` may still read them.
static int pld_correct_dev(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                           const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                           int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, const double *y,
                           const double *err, const uint8_t *cadence_mask, double clip_sigma, int niters, double *X,
                           double *prior_sigma, double *prior_mu, double *w, double *model, uint8_t *outlier,
                           double *spline_part, double *corrected, void *stream, const int32_t *p_count,
                           const int32_t *pb_count) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && N >= 2 && P >= 0 && Pb >= 1 && K >= 1, "bad shapes");
    LK_REQUIRE(bkg_pix && lc_flux && time && knots && y && w && model && outlier, "NULL buffer");
    LK_REQUIRE(X && prior_sigma && prior_mu, "NULL scratch (X: B x N x K, prior_sigma and prior_mu: B x K doubles)");
    LK_REQUIRE(n_knots + 1 <= K, "K=%d is narrower than the spline block (%d columns)", K, n_knots + 1);
    LK_HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool has_pld = P > 0 && pld_pix != nullptr;
    if (!has_pld) p_count = nullptr;
    if (p_count || pb_count) {   // ragged: the counts come back for the check (the design launch synchronises the stream anyway)
        std::vector<int32_t> hc((size_t)2 * B);
        if (p_count) LK_HIP_CHECK(hipMemcpyAsync(hc.data(), p_count, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        if (pb_count) LK_HIP_CHECK(hipMemcpyAsync(hc.data() + B, pb_count, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        LK_HIP_CHECK(hipStreamSynchronize(st));
        int rc_ = pld_check_counts("PLD", p_count ? hc.data() : nullptr, B, P, pca_components);
        if (!rc_) rc_ = pld_check_counts("background", pb_count ? hc.data() + B : nullptr, B, Pb, pca_components);
        if (rc_) return rc_;
    }
    LK_HIP_CHECK(hipMemsetAsync(prior_mu, 0, (size_t)B * K * 8, st));   // prior_mu = 0 for every PLD column
    int rc = lk::pld_design_launch(h, B, N, has_pld ? P : 0, Pb, has_pld ? pld_pix : nullptr, bkg_pix, lc_flux, time, knots,
                                   n_inner, pld_order, pca_components, n_knots, spline_degree, normalize_bkg, K, X, prior_sigma,
                                   st, p_count, pb_count);
    if (rc) return rc;
    std::vector<int64_t> off((size_t)B + 1);
    for (int b = 0; b <= B; ++b) off[b] = (int64_t)b * N;
    rc = lk::regress_launch(h, B, off.data(), K, X, y, err, cadence_mask, prior_mu, prior_sigma, clip_sigma, niters, w, model,
                            outlier, st);
    if (rc) return rc;
    if (spline_part) {
        rc = lk::model_part_launch(h, B, N, K, K - (n_knots + 1), K, X, w, spline_part, st);
        if (rc) return rc;
    }
    if (corrected) return lk::pld_corrected_launch(h, B, N, y, model, spline_part, corrected, st);
    return LK_OK;
}

int lk_pld_correct_batch_dev(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                             const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                             int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K, const double *y,
                             const double *err, const uint8_t *cadence_mask, double clip_sigma, int niters, double *X,
                             double *prior_sigma, double *prior_mu, double *w, double *model, uint8_t *outlier,
                             double *spline_part, double *corrected, void *stream) {
    return pld_correct_dev(h, B, N, P, Pb, pld_pix, bkg_pix, lc_flux, time, knots, n_inner, pld_order, pca_components, n_knots,
                           spline_degree, normalize_bkg, K, y, err, cadence_mask, clip_sigma, niters, X, prior_sigma, prior_mu, w,
                           model, outlier, spline_part, corrected, stream, nullptr, nullptr);
}

// lk_pld_correct_batch_dev for ragged pixel blocks: p_count / pb_count are DEVICE arrays of B entries (NULL = every column).
int lk_pld_correct_ragged_batch_dev(lk_handle *h, int B, int N, int P, int Pb, const float *pld_pix, const float *bkg_pix,
                                    const float *lc_flux, const double *time, const double *knots, int n_inner, int pld_order,
                                    int pca_components, int n_knots, int spline_degree, int normalize_bkg, int K,
                                    const double *y, const double *err, const uint8_t *cadence_mask, double clip_sigma,
                                    int niters, double *X, double *prior_sigma, double *prior_mu, double *w, double *model,
                                    uint8_t *outlier, double *spline_part, double *corrected, void *stream,
                                    const int32_t *p_count, const int32_t *pb_count) {
    return pld_correct_dev(h, B, N, P, Pb, pld_pix, bkg_pix, lc_flux, time, knots, n_inner, pld_order, pca_components, n_knots,
                           spline_degree, normalize_bkg, K, y, err, cadence_mask, clip_sigma, niters, X, prior_sigma, prior_mu, w,
                           model, outlier, spline_part, corrected, stream, p_count, pb_count);
}

// ------------------------------------------------------------------------------------------------ resident pixel cubes
int lk_cube_aperture_batch_dev(lk_handle *h, int B, int N, int npix, const float *flux, const float *flux_err,
                               const uint8_t *mask, int mask_stride, float *flux_out, float *err_out, uint8_t *keep_out,
                               int64_t *kept_host, int64_t *nonfinite_host, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_aperture_launch(h, B, N, npix, flux, flux_err, mask, mask_stride, flux_out, err_out, keep_out, kept_host,
                                    nonfinite_host, static_cast<hipStream_t>(stream));
}

int lk_cube_median_image_batch_dev(lk_handle *h, int B, int N, int npix, const float *cube, const uint8_t *keep,
                                   double *median, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_median_image_launch(h, B, N, npix, cube, keep, median, static_cast<hipStream_t>(stream));
}

int lk_pld_gather_batch_dev(lk_handle *h, int B, int N, int npix, int n, const float *cube, const double *time,
                            const float *flux32, const float *err32, const uint8_t *keep, int P, const int32_t *pld_idx_host,
                            int pld_idx_stride, int Pb, const int32_t *bkg_idx_host, int bkg_idx_stride, int n_inner,
                            const int32_t *knot_lo_host, const double *knot_g_host, double *t_out, double *y_out,
                            double *err_out, float *lcf_out, float *pld_out, float *bkg_out, double *knots_out,
                            int *nonfinite_host, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pld_gather_launch(h, B, N, npix, n, cube, time, flux32, err32, keep, P, pld_idx_host, pld_idx_stride, Pb,
                                 bkg_idx_host, bkg_idx_stride, n_inner, knot_lo_host, knot_g_host, t_out, y_out, err_out,
                                 lcf_out, pld_out, bkg_out, knots_out, nonfinite_host, static_cast<hipStream_t>(stream));
}

int lk_cube_threshold_mask_batch_dev(lk_handle *h, int B, int ny, int nx, const double *median, double threshold, int use_ref,
                                     double ref_col, double ref_row, int invert, uint8_t *mask, int32_t *count, int32_t *idx,
                                     void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_threshold_mask_launch(h, B, ny, nx, median, threshold, use_ref, ref_col, ref_row, invert, mask, count, idx,
                                          static_cast<hipStream_t>(stream));
}

int lk_pld_gather_ragged_batch_dev(lk_handle *h, int B, int N, int npix, int n, const float *cube, const double *time,
                                   const float *flux32, const float *err32, const uint8_t *keep, int P, const int32_t *pld_idx,
                                   int pld_idx_stride, int Pb, const int32_t *bkg_idx, int bkg_idx_stride, int n_inner,
                                   const int32_t *knot_lo_host, const double *knot_g_host, double *t_out, double *y_out,
                                   double *err_out, float *lcf_out, float *pld_out, float *bkg_out, double *knots_out,
                                   int *nonfinite_host, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE((P == 0 || pld_idx) && (Pb == 0 || bkg_idx), "the ragged gather needs a device index list per block");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::pld_gather_launch(h, B, N, npix, n, cube, time, flux32, err32, keep, P, nullptr, pld_idx_stride, Pb, nullptr,
                                 bkg_idx_stride, n_inner, knot_lo_host, knot_g_host, t_out, y_out, err_out, lcf_out, pld_out,
                                 bkg_out, knots_out, nonfinite_host, static_cast<hipStream_t>(stream), pld_idx, bkg_idx);
}

// ------------------------------------------------------------------------------------------------ design-matrix operations
int lk_pca_batch_dev(lk_handle *h, int B, int N, int P, int k, const double *A, double *U, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::dm_pca_launch(h, B, N, P, k, A, U, static_cast<hipStream_t>(stream));
}

int lk_pca_batch(lk_handle *h, int B, int N, int P, int k, const double *A, double *U) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && N >= 1 && P >= 1 && k >= 1 && A && U, "bad arguments");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const double *dA;
    double *dU;
    lk::StagedCall io(h);
    int rc = io.in(dA, A, (size_t)B * N * P).out(dU, U, (size_t)B * N * k).stage();
    if (rc) return rc;
    rc = lk::dm_pca_launch(h, B, N, P, k, dA, dU, nullptr);
    return rc ? rc : io.finish();
}

int lk_spline_basis_batch_dev(lk_handle *h, int B, int N, const double *x, const double *knots, int n_inner, int degree,
                              double *out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::dm_spline_launch(h, B, N, x, knots, n_inner, degree, out, static_cast<hipStream_t>(stream));
}

int lk_spline_basis_batch(lk_handle *h, int B, int N, const double *x, const double *knots, int n_inner, int degree,
                          double *out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && N >= 1 && n_inner >= 0 && degree >= 0 && x && knots && out, "bad arguments");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const double *dx, *dk;
    double *dout;
    lk::StagedCall io(h);
    int rc = io.in(dx, x, (size_t)B * N).in(dk, knots, (size_t)B * (n_inner + 2))
                 .out(dout, out, (size_t)B * N * (n_inner + degree + 1)).stage();
    if (rc) return rc;
    rc = lk::dm_spline_launch(h, B, N, dx, dk, n_inner, degree, dout, nullptr);
    return rc ? rc : io.finish();
}

int lk_standardize_batch_dev(lk_handle *h, int B, int N, int P, const double *A, double *out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::dm_standardize_launch(h, B, N, P, A, out, static_cast<hipStream_t>(stream));
}

int lk_standardize_batch(lk_handle *h, int B, int N, int P, const double *A, double *out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && N >= 1 && P >= 1 && A && out, "bad arguments");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t n = (size_t)B * N * P;
    const double *dA;
    double *dO;
    lk::StagedCall io(h);
    int rc = io.in(dA, A, n).out(dO, out, n).stage();
    if (rc) return rc;
    rc = lk::dm_standardize_launch(h, B, N, P, dA, dO, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ pinned host memory
int lk_host_alloc(void **ptr, size_t bytes) {
    LK_REQUIRE(ptr != nullptr, "ptr is NULL");
    *ptr = nullptr;
    LK_HIP_CHECK(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return LK_OK;
}

int lk_host_free(void *ptr) {
    if (ptr) LK_HIP_CHECK(hipHostFree(ptr));
    return LK_OK;
}

// ------------------------------------------------------------------------------------------------ LS 'fast' + peaks
int lk_ls_fast_peaks_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *y,
                               const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                               int normalization, const double *scale, int oversampling, double *power,
                               double *max_power, int64_t *argmax, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(power != nullptr, "power must be non-NULL for the device flavour (the spectra stay in HBM anyway)");
    LK_HIP_CHECK(hipSetDevice(h->device));
    // the per-target (max power, argmax) come out of the fused FFT step itself (no second pass over the spectra)
    return lk::lsfast_launch(h, B, n_off_host, t, y, dy, f0, df, M, fit_mean, center_data, normalization, scale,
                             oversampling, power, static_cast<hipStream_t>(stream), max_power, argmax);
}

extern "C++" {
static int pipeline_init(lk_handle *h) {
    if (h->s_in) return LK_OK;
    LK_HIP_CHECK(hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
    LK_HIP_CHECK(hipStreamCreateWithFlags(&h->s_comp, hipStreamNonBlocking));
    LK_HIP_CHECK(hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        LK_HIP_CHECK(hipEventCreateWithFlags(&h->ev_in[i], hipEventDisableTiming));
        LK_HIP_CHECK(hipEventCreateWithFlags(&h->ev_comp[i], hipEventDisableTiming));
        LK_HIP_CHECK(hipEventCreateWithFlags(&h->ev_out[i], hipEventDisableTiming));
    }
    return LK_OK;
}
}  // extern "C++"

// Host-pointer flavour, software-pipelined over chunks of targets: the H2D copy of chunk k+1 (stream s_in), the
// kernels of chunk k (s_comp) and the D2H copy of chunk k-1 (s_out) overlap; both device buffers are double
// buffered and ordered by events.  Caller buffers that are pinned (lk_host_alloc / hipHostMalloc / hipHostRegister)
// are DMA'd directly and the whole loop is asynchronous; pageable buffers go through the runtime's own staging
// (the host blocks inside each copy, the kernels of the next chunk are already queued).  power may be NULL
// (peaks only: the 8 B x B x M of spectra never cross PCIe); max_power / argmax may both be NULL.
extern "C++" {
// astropy hands LombScargle times relative to the first cadence of each light curve (lombscargle/core.py:119-126: trel =
// t - t[0]); a packed batch holds absolute times.  One workgroup per target: every lane reads t[lo] BEFORE the barrier, so
// the in-place subtraction is the same fp64 `t - t[0]` numpy does, 40 us for 160 MB instead of a host pass.
__global__ __launch_bounds__(1024) void lc_rebase_kernel(double *__restrict__ t, const int64_t *__restrict__ off,
                                                         int64_t base) {
    const int64_t lo = off[blockIdx.x] - base, n = off[blockIdx.x + 1] - off[blockIdx.x];
    if (n <= 0) return;
    const double t0 = t[lo];
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += 1024) t[lo + i] -= t0;
}

static int ls_fast_peaks_host(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y,
                              const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                              int normalization, const double *scale, int oversampling, double *power,
                              double *max_power, int64_t *argmax, bool rebase);
}  // extern "C++"

int lk_ls_fast_peaks_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y,
                           const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                           int normalization, const double *scale, int oversampling, double *power,
                           double *max_power, int64_t *argmax) {
    return ls_fast_peaks_host(h, B, n_off, t, y, dy, f0, df, M, fit_mean, center_data, normalization, scale, oversampling,
                              power, max_power, argmax, false);
}

int lk_ls_fast_peaks_lc_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux,
                              const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                              int normalization, const double *scale, int oversampling, double *power,
                              double *max_power, int64_t *argmax) {
    return ls_fast_peaks_host(h, B, n_off, time, flux, dy, f0, df, M, fit_mean, center_data, normalization, scale,
                              oversampling, power, max_power, argmax, true);
}

extern "C++" {
static int ls_fast_peaks_host(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *y,
                              const double *dy, double f0, double df, int64_t M, int fit_mean, int center_data,
                              int normalization, const double *scale, int oversampling, double *power,
                              double *max_power, int64_t *argmax, bool rebase) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    LK_REQUIRE(M >= 0, "M must be >= 0");
    if (B == 0 || M == 0) return LK_OK;
    LK_REQUIRE(t && y, "t, y must be non-NULL");
    LK_REQUIRE(power || (max_power && argmax), "nothing to compute: power, max_power and argmax are all NULL");
    LK_REQUIRE((max_power == nullptr) == (argmax == nullptr), "max_power and argmax must both be given (or both NULL)");
    LK_REQUIRE(n_off[0] == 0, "n_off[0] must be 0");
    for (int b = 0; b < B; ++b) LK_REQUIRE(n_off[b + 1] >= n_off[b], "n_off must be non-decreasing");
    LK_HIP_CHECK(hipSetDevice(h->device));
    int rc = pipeline_init(h);
    if (rc) return rc;
    // chunk = as many targets as give ~64 MiB of spectra (large enough to amortise launches, small enough to pipeline)
    const size_t chunk_mb = (size_t)std::max(1, h->host_chunk_mb);
    const int C = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (chunk_mb << 20) / ((size_t)M * 8)));
    const int nchunks = (B + C - 1) / C;
    size_t in_max = 0;
    for (int k = 0; k < nchunks; ++k) {
        const int b0 = k * C, b1 = std::min(B, b0 + C);
        in_max = std::max(in_max, (size_t)(n_off[b1] - n_off[b0]));
    }
    const int narr = dy ? 3 : 2;
    double *d_in[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    double *d_pow[2], *d_scale, *d_max;
    int64_t *d_arg, *d_off_all;
    lk::Scratch ws(h, h->staging);
    for (int s = 0; s < 2; ++s) {
        for (int a = 0; a < narr; ++a) ws.buf(d_in[s][a], in_max);
        ws.buf(d_pow[s], (size_t)C * M);
    }
    ws.buf(d_scale, B, scale != nullptr)
        .buf(d_max, B, max_power != nullptr)
        .buf(d_arg, B, argmax != nullptr)
        .buf(d_off_all, B + 1, rebase);
    if ((rc = ws.carve(h->s_in))) return rc;
    if (scale) LK_HIP_CHECK(hipMemcpyAsync(d_scale, scale, (size_t)B * 8, hipMemcpyHostToDevice, h->s_in));
    if (rebase) LK_HIP_CHECK(hipMemcpyAsync(d_off_all, n_off, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, h->s_in));
    std::vector<int64_t> offc((size_t)C + 1);

    auto enqueue_in = [&](int k) -> int {
        const int s = k & 1, b0 = k * C, b1 = std::min(B, b0 + C);
        const size_t lo = (size_t)n_off[b0], nbytes = (size_t)(n_off[b1] - n_off[b0]) * 8;
        if (k >= 2) LK_HIP_CHECK(hipStreamWaitEvent(h->s_in, h->ev_comp[s], 0));  // kernels of chunk k-2 are done with d_in[s]
        if (nbytes) {
            LK_HIP_CHECK(hipMemcpyAsync(d_in[s][0], t + lo, nbytes, hipMemcpyHostToDevice, h->s_in));
            LK_HIP_CHECK(hipMemcpyAsync(d_in[s][1], y + lo, nbytes, hipMemcpyHostToDevice, h->s_in));
            if (dy) LK_HIP_CHECK(hipMemcpyAsync(d_in[s][2], dy + lo, nbytes, hipMemcpyHostToDevice, h->s_in));
        }
        LK_HIP_CHECK(hipEventRecord(h->ev_in[s], h->s_in));
        return LK_OK;
    };
    auto enqueue_comp = [&](int k) -> int {
        const int s = k & 1, b0 = k * C, b1 = std::min(B, b0 + C), nb = b1 - b0;
        LK_HIP_CHECK(hipStreamWaitEvent(h->s_comp, h->ev_in[s], 0));
        if (k >= 2 && power) LK_HIP_CHECK(hipStreamWaitEvent(h->s_comp, h->ev_out[s], 0));  // D2H of chunk k-2 has left d_pow[s]
        for (int b = 0; b <= nb; ++b) offc[b] = n_off[b0 + b] - n_off[b0];
        if (rebase)  // ordered behind the copy of d_off_all by ev_in (both on s_in)
            hipLaunchKernelGGL(lc_rebase_kernel, dim3(nb), dim3(1024), 0, h->s_comp, d_in[s][0], d_off_all + b0, n_off[b0]);
        int r = lk::lsfast_launch(h, nb, offc.data(), d_in[s][0], d_in[s][1], dy ? d_in[s][2] : nullptr, f0, df, M,
                                  fit_mean, center_data, normalization, d_scale ? d_scale + b0 : nullptr, oversampling,
                                  d_pow[s], h->s_comp);
        if (r) return r;
        if (d_max) {
            r = lk::argmax_launch(h, nb, M, d_pow[s], d_max + b0, d_arg + b0, h->s_comp);
            if (r) return r;
        }
        LK_HIP_CHECK(hipEventRecord(h->ev_comp[s], h->s_comp));
        return LK_OK;
    };
    auto enqueue_out = [&](int k) -> int {
        if (!power) return LK_OK;
        const int s = k & 1, b0 = k * C, b1 = std::min(B, b0 + C);
        LK_HIP_CHECK(hipStreamWaitEvent(h->s_out, h->ev_comp[s], 0));
        LK_HIP_CHECK(hipMemcpyAsync(power + (size_t)b0 * (size_t)M, d_pow[s], (size_t)(b1 - b0) * (size_t)M * 8,
                                    hipMemcpyDeviceToHost, h->s_out));
        LK_HIP_CHECK(hipEventRecord(h->ev_out[s], h->s_out));
        return LK_OK;
    };
    // the pipeline: chunk k+1 is copied in and its kernels are queued BEFORE the copy-out of chunk k is issued, so a
    // blocking (pageable) copy-out never leaves the GPU without queued work
    if ((rc = enqueue_in(0)) || (rc = enqueue_comp(0))) goto fail;
    for (int k = 0; k < nchunks; ++k) {
        if (k + 1 < nchunks && ((rc = enqueue_in(k + 1)) || (rc = enqueue_comp(k + 1)))) goto fail;
        if ((rc = enqueue_out(k))) goto fail;
    }
    if (d_max) {
        LK_HIP_CHECK(hipMemcpyAsync(max_power, d_max, (size_t)B * 8, hipMemcpyDeviceToHost, h->s_comp));
        LK_HIP_CHECK(hipMemcpyAsync(argmax, d_arg, (size_t)B * 8, hipMemcpyDeviceToHost, h->s_comp));
    }
    LK_HIP_CHECK(hipStreamSynchronize(h->s_in));
    LK_HIP_CHECK(hipStreamSynchronize(h->s_comp));
    LK_HIP_CHECK(hipStreamSynchronize(h->s_out));
    return LK_OK;
fail:
    (void)hipStreamSynchronize(h->s_in);
    (void)hipStreamSynchronize(h->s_comp);
    (void)hipStreamSynchronize(h->s_out);
    return rc;
}
}  // extern "C++"

// ------------------------------------------------------------------------------------------------ sigma clip
int lk_sigma_clip_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *y, double sigma, int maxiters,
                            uint8_t *outlier, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::sigma_clip_launch(h, B, n_off_host, y, sigma, maxiters, outlier, static_cast<hipStream_t>(stream));
}

int lk_sigma_clip_batch(lk_handle *h, int B, const int64_t *n_off, const double *y, double sigma, int maxiters,
                        uint8_t *outlier) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0 || n_off[B] == 0) return LK_OK;
    LK_REQUIRE(y && outlier, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dy;
    uint8_t *dm;
    lk::StagedCall io(h);
    int rc = io.in(dy, y, ntot).out(dm, outlier, ntot).stage();
    if (rc) return rc;
    rc = lk::sigma_clip_launch(h, B, n_off, dy, sigma, maxiters, dm, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ select.hip
int lk_outlier_mask_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *y, double sigma_lower,
                              double sigma_upper, int maxiters, uint8_t *outlier, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::outlier_mask_launch(h, B, n_off_host, y, sigma_lower, sigma_upper, maxiters, outlier,
                                   static_cast<hipStream_t>(stream));
}

int lk_outlier_mask_batch(lk_handle *h, int B, const int64_t *n_off, const double *y, double sigma_lower, double sigma_upper,
                          int maxiters, uint8_t *outlier) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0 || n_off[B] == 0) return LK_OK;
    LK_REQUIRE(n_off[0] == 0 && n_off[B] > 0, "n_off must be prefix offsets starting at 0");
    LK_REQUIRE(y && outlier, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dy;
    uint8_t *dm;
    lk::StagedCall io(h);
    int rc = io.in(dy, y, ntot).out(dm, outlier, ntot).stage();
    if (rc) return rc;
    rc = lk::outlier_mask_launch(h, B, n_off, dy, sigma_lower, sigma_upper, maxiters, dm, nullptr);
    return rc ? rc : io.finish();
}

int lk_select_columns_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const uint8_t *mask, int invert, int ncols,
                                const int *elem_bytes, const void *const *cols_in, void *const *cols_out,
                                int64_t *new_off_host, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::select_columns_launch(h, B, n_off_host, mask, invert, ncols, elem_bytes, cols_in, cols_out, new_off_host,
                                     static_cast<hipStream_t>(stream));
}

int lk_cdpp_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *flat_flux, const uint8_t *outlier,
                      int transit_duration, double *cdpp_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cdpp_launch(h, B, n_off_host, flat_flux, outlier, transit_duration, cdpp_out, static_cast<hipStream_t>(stream));
}

int lk_cdpp_batch(lk_handle *h, int B, const int64_t *n_off, const double *flat_flux, const uint8_t *outlier,
                  int transit_duration, double *cdpp_out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    LK_REQUIRE(transit_duration >= 1, "transit_duration must be >= 1 cadence (got %d)", transit_duration);
    if (B == 0) return LK_OK;
    LK_REQUIRE(n_off[0] == 0 && n_off[B] >= 0, "n_off must be prefix offsets starting at 0");
    LK_REQUIRE(cdpp_out != nullptr && (flat_flux != nullptr || n_off[B] == 0), "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *df;
    const uint8_t *dm;
    double *dc;
    lk::StagedCall io(h);
    int rc = io.in(df, flat_flux, ntot).in(dm, outlier, ntot).out(dc, cdpp_out, (size_t)B).stage();
    if (rc) return rc;
    rc = lk::cdpp_launch(h, B, n_off, df, dm, transit_duration, dc, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ fillgaps.hip
int lk_fill_gaps_plan_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                                const int32_t *cadenceno, double *stats, int32_t *pos, int64_t *new_off_host, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fill_gaps_plan_launch(h, B, n_off_host, time, flux, cadenceno, stats, pos, new_off_host, static_cast<hipStream_t>(stream));
}

int lk_fill_gaps_plan_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux, const int32_t *cadenceno,
                            double *stats, int32_t *pos, int64_t *new_off) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr && new_off != nullptr, "bad batch description");
    if (B == 0) {
        new_off[0] = 0;
        return LK_OK;
    }
    LK_REQUIRE(n_off[0] == 0 && n_off[B] >= 0, "n_off must be prefix offsets starting at 0");
    LK_REQUIRE(stats != nullptr && ((time && flux && pos) || n_off[B] == 0), "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *df;
    const int32_t *dc;
    double *ds;
    int32_t *dp;
    lk::StagedCall io(h);
    int rc = io.in(dt, time, ntot).in(df, flux, ntot).in(dc, cadenceno, ntot).out(ds, stats, (size_t)B * 4).out(dp, pos, ntot).stage();
    if (rc) return rc;
    rc = lk::fill_gaps_plan_launch(h, B, n_off, dt, df, dc, ds, dp, new_off, nullptr);
    return rc ? rc : io.finish();
}

int lk_fill_gaps_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const int64_t *new_off_host, const double *time,
                           const double *flux, const double *flux_err, const int32_t *quality, const int32_t *cadenceno,
                           const double *stats, const int32_t *pos, const double *noise_mean, const double *noise_std, uint64_t seed,
                           int64_t first_target, int64_t stream_id, double *time_out, double *flux_out, double *flux_err_out,
                           int32_t *quality_out, int32_t *cadenceno_out, uint8_t *inserted, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fill_gaps_launch(h, B, n_off_host, new_off_host, time, flux, flux_err, quality, cadenceno, stats, pos, noise_mean,
                                noise_std, seed, first_target, stream_id, time_out, flux_out, flux_err_out, quality_out,
                                cadenceno_out, inserted, static_cast<hipStream_t>(stream));
}

int lk_fill_gaps_batch(lk_handle *h, int B, const int64_t *n_off, const int64_t *new_off, const double *time, const double *flux,
                       const double *flux_err, const int32_t *quality, const int32_t *cadenceno, const double *stats,
                       const int32_t *pos, const double *noise_mean, const double *noise_std, uint64_t seed, int64_t first_target,
                       int64_t stream_id, double *time_out, double *flux_out, double *flux_err_out, int32_t *quality_out,
                       int32_t *cadenceno_out, uint8_t *inserted) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr && new_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(n_off[0] == 0 && n_off[B] >= 0 && new_off[0] == 0 && new_off[B] >= n_off[B], "n_off / new_off must be prefix offsets starting at 0");
    if (new_off[B] == 0) return LK_OK;
    LK_REQUIRE(stats && noise_mean && noise_std && time && flux && pos && time_out && flux_out && inserted, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], nnew = (size_t)new_off[B];
    const double *dt, *df, *de, *ds, *dm, *dn;
    const int32_t *dq, *dc, *dp;
    double *ot, *of, *oe;
    int32_t *oq, *oc;
    uint8_t *om;
    lk::StagedCall io(h);
    int rc = io.in(dt, time, ntot).in(df, flux, ntot).in(de, flux_err, ntot).in(dq, quality, ntot).in(dc, cadenceno, ntot)
                 .in(ds, stats, (size_t)B * 4).in(dp, pos, ntot).in(dm, noise_mean, (size_t)B).in(dn, noise_std, (size_t)B)
                 .out(ot, time_out, nnew).out(of, flux_out, nnew).out(oe, flux_err_out, nnew).out(oq, quality_out, nnew)
                 .out(oc, cadenceno_out, nnew).out(om, inserted, nnew).stage();
    if (rc) return rc;
    rc = lk::fill_gaps_launch(h, B, n_off, new_off, dt, df, de, dq, dc, ds, dp, dm, dn, seed, first_target, stream_id, ot, of, oe, oq,
                              oc, om, nullptr);
    return rc ? rc : io.finish();
}

int lk_gather_segments_batch_dev(lk_handle *h, int S, const int64_t *src_start_host, const int64_t *dst_off_host, int64_t n_src,
                                 int ncols, const int *elem_bytes, const void *const *cols_in, void *const *cols_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::gather_segments_launch(h, S, src_start_host, dst_off_host, n_src, ncols, elem_bytes, cols_in, cols_out,
                                      static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ batch ingest (N4)
int lk_ingest_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                        const double *flux_err, int normalize, double *t_out, double *flux_out, double *flux_err_out,
                        int64_t *new_off_host, double *median_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::ingest_launch(h, B, n_off_host, t, flux, flux_err, normalize, t_out, flux_out, flux_err_out, new_off_host,
                             median_out, static_cast<hipStream_t>(stream));
}

int lk_ingest_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                    int normalize, double *t_out, double *flux_out, double *flux_err_out, int64_t *new_off,
                    double *median_out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr && new_off != nullptr, "bad batch description");
    if (B == 0) {
        new_off[0] = 0;
        return LK_OK;
    }
    LK_REQUIRE(t && flux && t_out && flux_out, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const int64_t *kept = &new_off[B];  // set by the launch
    const double *dt, *df, *de;
    double *dto, *dfo, *deo, *dmed;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(df, flux, ntot).in(de, flux_err, ntot).out(dto, t_out, ntot, kept)
                 .out(dfo, flux_out, ntot, kept).out(deo, flux_err_out, ntot, kept).out(dmed, median_out, (size_t)B).stage();
    if (rc) return rc;
    rc = lk::ingest_launch(h, B, n_off, dt, df, de, normalize, dto, dfo, deo, new_off, dmed, nullptr);
    return rc ? rc : io.finish();
}

int lk_fits_unpack_batch_dev(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off_host, const int32_t *desc_host,
                             const int64_t *bitmask_host, double *t_out, double *flux_out, double *flux_err_out,
                             int32_t *quality_out, int64_t *new_off_host, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fits_unpack_launch(h, B, raw, raw_off_host, desc_host, bitmask_host, t_out, flux_out, flux_err_out,
                                  quality_out, new_off_host, static_cast<hipStream_t>(stream));
}

int lk_fits_unpack_batch(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off, const int32_t *desc,
                         const int64_t *bitmask, double *t_out, double *flux_out, double *flux_err_out,
                         int32_t *quality_out, int64_t *new_off) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && raw_off != nullptr && desc != nullptr && new_off != nullptr, "bad batch description");
    if (B == 0) {
        new_off[0] = 0;
        return LK_OK;
    }
    LK_REQUIRE(raw && bitmask && t_out && flux_out, "NULL buffer");
    LK_REQUIRE(raw_off[0] == 0, "raw_off[0] must be 0");
    LK_HIP_CHECK(hipSetDevice(h->device));
    size_t rows = 0;
    for (int b = 0; b < B; ++b) rows += (size_t)std::max(0, desc[(size_t)b * 10 + 1]);
    const int64_t *kept = &new_off[B];  // set by the launch
    const uint8_t *draw;
    double *dto, *dfo, *deo;
    int32_t *dqo;
    lk::StagedCall io(h);
    int rc = io.in(draw, raw, (size_t)raw_off[B], 16).out(dto, t_out, rows, kept).out(dfo, flux_out, rows, kept)
                 .out(deo, flux_err_out, rows, kept).out(dqo, quality_out, rows, kept).stage();
    if (rc) return rc;
    rc = lk::fits_unpack_launch(h, B, draw, raw_off, desc, bitmask, dto, dfo, deo, dqo, new_off, nullptr);
    return rc ? rc : io.finish();
}

int lk_fits_cadenceno_batch_dev(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off_host, const int32_t *desc_host,
                                const int32_t *col_host, const int64_t *bitmask_host, const int64_t *new_off_host,
                                int32_t *cadenceno_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fits_int_column_launch(h, B, raw, raw_off_host, desc_host, col_host, bitmask_host, new_off_host, cadenceno_out,
                                      static_cast<hipStream_t>(stream));
}

int lk_fits_cadenceno_batch(lk_handle *h, int B, const uint8_t *raw, const int64_t *raw_off, const int32_t *desc,
                            const int32_t *col, const int64_t *bitmask, const int64_t *new_off, int32_t *cadenceno_out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && raw_off != nullptr && desc != nullptr && col != nullptr && new_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(raw && bitmask && cadenceno_out, "NULL buffer");
    LK_REQUIRE(raw_off[0] == 0 && raw_off[B] >= 0 && new_off[B] >= 0, "raw_off[0] must be 0");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const uint8_t *draw;
    int32_t *dco;
    lk::StagedCall io(h);
    int rc = io.in(draw, raw, (size_t)raw_off[B]).out(dco, cadenceno_out, (size_t)new_off[B]).stage();
    if (rc) return rc;
    rc = lk::fits_int_column_launch(h, B, draw, raw_off, desc, col, bitmask, new_off, dco, nullptr);
    return rc ? rc : io.finish();
}

int lk_fits_unpack_cube_dev(lk_handle *h, const uint8_t *raw, int row_bytes, int n_rows, int off_time, int code_time,
                            int off_quality, int code_quality, int64_t bitmask, int keep_nan_time, int ncols,
                            const int32_t *col_off_host, int npix, double *t_out, int32_t *quality_out, float *cubes_out,
                            int64_t *kept_host, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fits_cube_launch(h, raw, row_bytes, n_rows, off_time, code_time, off_quality, code_quality, bitmask,
                                keep_nan_time, ncols, col_off_host, npix, t_out, quality_out, cubes_out, kept_host,
                                static_cast<hipStream_t>(stream));
}

int lk_fits_unpack_cube(lk_handle *h, const uint8_t *raw, int row_bytes, int n_rows, int off_time, int code_time,
                        int off_quality, int code_quality, int64_t bitmask, int keep_nan_time, int ncols,
                        const int32_t *col_off, int npix, double *t_out, int32_t *quality_out, float *cubes_out,
                        int64_t *kept) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(raw && col_off && t_out && cubes_out && kept, "NULL buffer");
    LK_REQUIRE(row_bytes >= 1 && n_rows >= 0 && ncols >= 1 && ncols <= 4 && npix >= 1, "bad table description");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const uint8_t *draw;
    double *dt;
    int32_t *dq;
    float *dc;
    lk::StagedCall io(h);
    // 16 bytes of tail past raw and the cubes, 8 past the times and the quality flags
    int rc = io.in(draw, raw, (size_t)row_bytes * n_rows, 16).out(dt, t_out, (size_t)n_rows + 1, kept)
                 .out(dq, quality_out, (size_t)n_rows + 2, kept).scratch(dc, (size_t)ncols * n_rows * npix + 4).stage();
    if (rc) return rc;
    rc = lk::fits_cube_launch(h, draw, row_bytes, n_rows, off_time, code_time, off_quality, code_quality, bitmask,
                              keep_nan_time, ncols, col_off, npix, dt, dq, dc, kept, nullptr);
    if (rc) return rc;
    LK_HIP_CHECK(hipDeviceSynchronize());
    rc = io.finish();
    if (rc) return rc;
    const size_t k = (size_t)*kept;
    for (int c = 0; c < ncols; ++c)  // host layout: [column][kept cadence][pixel], columns n_rows * npix apart like the device's
        LK_HIP_CHECK(hipMemcpy(cubes_out + (size_t)c * n_rows * npix, dc + (size_t)c * n_rows * npix, k * npix * 4,
                               hipMemcpyDeviceToHost));
    return LK_OK;
}

int lk_transit_mask_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const int32_t *planet_off,
                              const double *period, const double *duration, const double *transit_time, uint8_t *mask,
                              void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::transit_mask_launch(h, B, n_off_host, t, planet_off, period, duration, transit_time, mask,
                                   static_cast<hipStream_t>(stream));
}

int lk_transit_mask_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const int32_t *planet_off,
                          const double *period, const double *duration, const double *transit_time, uint8_t *mask) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0 || n_off[B] == 0) return LK_OK;
    LK_REQUIRE(t && mask, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt;
    uint8_t *dm;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).out(dm, mask, ntot).stage();
    if (rc) return rc;
    rc = lk::transit_mask_launch(h, B, n_off, dt, planet_off, period, duration, transit_time, dm, nullptr);
    return rc ? rc : io.finish();
}

int lk_bls_stats_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                           const double *ivar, const double *period, const double *duration, const double *transit_time,
                           const int64_t *tr_off_host, double *stats, int32_t *tr_first, int32_t *tr_n, int32_t *tr_count,
                           double *tr_ll, double *model, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::bls_stats_launch(h, B, n_off_host, time, flux, ivar, period, duration, transit_time, tr_off_host, stats, tr_first,
                                tr_n, tr_count, tr_ll, model, static_cast<hipStream_t>(stream));
}

int lk_bls_stats_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux, const double *ivar,
                       const double *period, const double *duration, const double *transit_time, const int64_t *tr_off,
                       double *stats, int32_t *tr_first, int32_t *tr_n, int32_t *tr_count, double *tr_ll, double *model) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr && tr_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(n_off[B] >= 0 && tr_off[B] >= 0, "bad batch description");
    LK_REQUIRE(n_off[B] == 0 || (time && flux), "NULL time or flux");
    LK_REQUIRE(stats && tr_first && tr_n && tr_count && tr_ll, "NULL output buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], ntr = (size_t)tr_off[B];
    const double *dt, *dy, *dw;
    double *dstats, *dll, *dmodel;
    int32_t *dfirst, *dn, *dcount;
    lk::StagedCall io(h);
    int rc = io.in(dt, time, ntot).in(dy, flux, ntot).in(dw, ivar, ntot).out(dstats, stats, (size_t)B * LK_BLS_NSTATS)
                 .out(dfirst, tr_first, (size_t)B).out(dn, tr_n, (size_t)B).out(dcount, tr_count, ntr).out(dll, tr_ll, ntr)
                 .out(dmodel, model, ntot).stage();
    if (rc) return rc;
    rc = lk::bls_stats_launch(h, B, n_off, dt, dy, dw, period, duration, transit_time, tr_off, dstats, dfirst, dn, dcount, dll,
                              dmodel, nullptr);
    return rc ? rc : io.finish();
}

int lk_ls_model_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                          const double *dy, const double *frequency, int nterms, int fit_mean, int center_data, int keep_mean,
                          double *theta, double *stats, double *model, double *residual, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::ls_model_launch(h, B, n_off_host, time, flux, dy, frequency, nterms, fit_mean, center_data, keep_mean, theta, stats,
                               model, residual, static_cast<hipStream_t>(stream));
}

int lk_ls_model_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux, const double *dy,
                      const double *frequency, int nterms, int fit_mean, int center_data, int keep_mean, double *theta,
                      double *stats, double *model, double *residual) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    LK_REQUIRE(nterms >= 1 && nterms <= 8, "nterms must be 1 .. 8 (got %d)", nterms);
    if (B == 0) return LK_OK;
    LK_REQUIRE(n_off[B] >= 0, "bad batch description");
    LK_REQUIRE(n_off[B] == 0 || (time && flux), "NULL time or flux");
    LK_REQUIRE(theta && stats, "NULL output buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *df, *de;
    double *dtheta, *dstats, *dmodel, *dres;
    lk::StagedCall io(h);
    int rc = io.in(dt, time, ntot).in(df, flux, ntot).in(de, dy, ntot).out(dtheta, theta, (size_t)B * (2 * nterms + 1))
                 .out(dstats, stats, (size_t)B * LK_LS_MODEL_NSTATS).out(dmodel, model, ntot).out(dres, residual, ntot).stage();
    if (rc) return rc;
    rc = lk::ls_model_launch(h, B, n_off, dt, df, de, frequency, nterms, fit_mean, center_data, keep_mean, dtheta, dstats, dmodel,
                             dres, nullptr);
    return rc ? rc : io.finish();
}

int lk_ls_model_eval_batch_dev(lk_handle *h, int B, const int64_t *m_off_host, const double *t_fit, const double *t_ref,
                               const double *frequency, int nterms, const double *theta, const double *stats, double *out,
                               void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::ls_model_eval_launch(h, B, m_off_host, t_fit, t_ref, frequency, nterms, theta, stats, out,
                                    static_cast<hipStream_t>(stream));
}

int lk_ls_model_eval_batch(lk_handle *h, int B, const int64_t *m_off, const double *t_fit, const double *t_ref,
                           const double *frequency, int nterms, const double *theta, const double *stats, double *out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && m_off != nullptr, "bad batch description");
    LK_REQUIRE(nterms >= 1 && nterms <= 8, "nterms must be 1 .. 8 (got %d)", nterms);
    if (B == 0 || m_off[B] == 0) return LK_OK;
    LK_REQUIRE(m_off[B] > 0 && t_fit && out, "NULL t_fit or out");
    LK_REQUIRE(theta && stats, "NULL fit parameters");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t mtot = (size_t)m_off[B];
    const double *dt, *dtheta, *dstats;
    double *dout;
    lk::StagedCall io(h);
    int rc = io.in(dt, t_fit, mtot).in(dtheta, theta, (size_t)B * (2 * nterms + 1)).in(dstats, stats, (size_t)B * LK_LS_MODEL_NSTATS)
                 .out(dout, out, mtot).stage();
    if (rc) return rc;
    rc = lk::ls_model_eval_launch(h, B, m_off, dt, t_ref, frequency, nterms, dtheta, dstats, dout, nullptr);
    return rc ? rc : io.finish();
}

int lk_bin_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                     const double *flux_err, const int64_t *bin_off, const double *time_bin_start, const double *edges_sec,
                     int64_t n_edges, double bin_size_sec, const uint8_t *has_err, double *t_out, double *flux_out,
                     double *flux_err_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::bin_launch(h, B, n_off_host, t, flux, flux_err, bin_off, time_bin_start, edges_sec, n_edges, bin_size_sec,
                          has_err, t_out, flux_out, flux_err_out, static_cast<hipStream_t>(stream));
}

int lk_bin_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                 const int64_t *bin_off, const double *time_bin_start, const double *edges_sec, int64_t n_edges,
                 double bin_size_sec, const uint8_t *has_err, double *t_out, double *flux_out, double *flux_err_out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr && bin_off != nullptr, "bad batch description");
    if (B == 0 || bin_off[B] == 0) return LK_OK;
    LK_REQUIRE(t && flux && t_out && flux_out && flux_err_out, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], nbin = (size_t)bin_off[B];
    const double *dt, *df, *de;
    double *dto, *dfo, *deo;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(df, flux, ntot).in(de, flux_err, ntot).out(dto, t_out, nbin).out(dfo, flux_out, nbin)
                 .out(deo, flux_err_out, nbin).stage();
    if (rc) return rc;
    rc = lk::bin_launch(h, B, n_off, dt, df, de, bin_off, time_bin_start, edges_sec, n_edges, bin_size_sec, has_err, dto, dfo,
                        deo, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ fold + bin by phase
int lk_fold_bin_plan_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                               const double *flux_err, const double *period, const double *epoch_time, int epoch_given,
                               double epoch_phase, const double *wrap_phase, int normalize_phase, const double *count_from,
                               double *plan, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fold_bin_plan_launch(h, B, n_off_host, t, flux, flux_err, period, epoch_time, epoch_given, epoch_phase, wrap_phase,
                                    normalize_phase, count_from, plan, static_cast<hipStream_t>(stream));
}

int lk_fold_bin_plan_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                           const double *period, const double *epoch_time, int epoch_given, double epoch_phase,
                           const double *wrap_phase, int normalize_phase, const double *count_from, double *plan) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && flux && plan, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *df, *de;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(df, flux, ntot).in(de, flux_err, ntot).stage();
    if (rc) return rc;
    return lk::fold_bin_plan_launch(h, B, n_off, dt, df, de, period, epoch_time, epoch_given, epoch_phase, wrap_phase,
                                    normalize_phase, count_from, plan, nullptr);
}

int lk_fold_cycle_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const int64_t *order,
                            const double *period, const double *cycle_epoch, const double *cycle_min, int64_t *cycle, uint8_t *odd,
                            uint8_t *even, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fold_cycle_launch(h, B, n_off_host, t, order, period, cycle_epoch, cycle_min, cycle, odd, even,
                                 static_cast<hipStream_t>(stream));
}

int lk_phase_bin_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *phase, const double *flux,
                           const double *flux_err, const uint8_t *sel, int sel_value, const int64_t *bin_off, const double *start,
                           const double *size_sec, const double *edges, const uint8_t *has_err, int median, double *phase_out,
                           double *flux_out, double *flux_err_out, int32_t *count_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::phase_bin_launch(h, B, n_off_host, phase, flux, flux_err, sel, sel_value, bin_off, start, size_sec, edges, has_err,
                                median, phase_out, flux_out, flux_err_out, count_out, static_cast<hipStream_t>(stream));
}

int lk_fold_bin_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                          const double *flux_err, const double *period, const double *epoch_time, double epoch_phase,
                          const double *wrap_phase, int normalize_phase, const double *cycle_epoch, const double *plan, int which,
                          const int64_t *bin_off, const double *start, const double *size_sec, const double *edges,
                          double *phase_out, double *flux_out, double *flux_err_out, int32_t *count_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::fold_bin_launch(h, B, n_off_host, t, flux, flux_err, period, epoch_time, epoch_phase, wrap_phase, normalize_phase,
                               cycle_epoch, plan, which, bin_off, start, size_sec, edges, phase_out, flux_out, flux_err_out,
                               count_out, static_cast<hipStream_t>(stream));
}

int lk_fold_bin_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                      const double *period, const double *epoch_time, double epoch_phase, const double *wrap_phase,
                      int normalize_phase, const double *cycle_epoch, const double *plan, int which, const int64_t *bin_off,
                      const double *start, const double *size_sec, const double *edges, double *phase_out, double *flux_out,
                      double *flux_err_out, int32_t *count_out) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr && bin_off != nullptr, "bad batch description");
    if (B == 0 || bin_off[B] == 0) return LK_OK;
    LK_REQUIRE(t && flux && phase_out && flux_out && flux_err_out && count_out, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], nbin = (size_t)bin_off[B];
    const double *dt, *df, *de;
    double *dpo, *dfo, *deo;
    int32_t *dco;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(df, flux, ntot).in(de, flux_err, ntot).out(dpo, phase_out, nbin).out(dfo, flux_out, nbin)
                 .out(deo, flux_err_out, nbin).out(dco, count_out, nbin).stage();
    if (rc) return rc;
    rc = lk::fold_bin_launch(h, B, n_off, dt, df, de, period, epoch_time, epoch_phase, wrap_phase, normalize_phase, cycle_epoch,
                             plan, which, bin_off, start, size_sec, edges, dpo, dfo, deo, dco, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ river diagrams
int lk_river_plan_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux,
                            const double *flux_err, const double *period, const double *epoch_time, int epoch_given, double *plan,
                            void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::river_plan_launch(h, B, n_off_host, t, flux, flux_err, period, epoch_time, epoch_given, plan,
                                 static_cast<hipStream_t>(stream));
}

int lk_river_plan_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                        const double *period, const double *epoch_time, int epoch_given, double *plan) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && flux && plan, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *df, *de;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(df, flux, ntot).in(de, flux_err, ntot).stage();
    if (rc) return rc;
    return lk::river_plan_launch(h, B, n_off, dt, df, de, period, epoch_time, epoch_given, plan, nullptr);
}

int lk_river_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *t, const double *flux, const double *flux_err,
                       const double *period, const double *epoch_time, const double *plan, int method, const int32_t *n_bins,
                       const int32_t *n_cycles, const int64_t *cell_off, const double *edges, double *river, int32_t *count,
                       int32_t *route, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::river_launch(h, B, n_off_host, t, flux, flux_err, period, epoch_time, plan, method, n_bins, n_cycles, cell_off, edges,
                            river, count, route, static_cast<hipStream_t>(stream));
}

int lk_river_batch(lk_handle *h, int B, const int64_t *n_off, const double *t, const double *flux, const double *flux_err,
                   const double *period, const double *epoch_time, const double *plan, int method, const int32_t *n_bins,
                   const int32_t *n_cycles, const int64_t *cell_off, const double *edges, double *river, int32_t *count,
                   int32_t *route) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr && cell_off != nullptr, "bad batch description");
    if (B == 0) return LK_OK;
    LK_REQUIRE(t && flux && river && count, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B], ncell = (size_t)cell_off[B];
    const double *dt, *df, *de;
    double *dro;
    int32_t *dco, *drt;
    lk::StagedCall io(h);
    int rc = io.in(dt, t, ntot).in(df, flux, ntot).in(de, flux_err, ntot).out(dro, river, ncell).out(dco, count, ncell)
                 .out(drt, route, (size_t)B).stage();
    if (rc) return rc;
    rc = lk::river_launch(h, B, n_off, dt, df, de, period, epoch_time, plan, method, n_bins, n_cycles, cell_off, edges, dro, dco,
                          drt, nullptr);
    return rc ? rc : io.finish();
}

// ------------------------------------------------------------------------------------------------ SFF
int lk_cube_centroids_batch_dev(lk_handle *h, int B, int N, int npix, int nx, const float *flux, const uint8_t *mask,
                                int mask_stride, double column0, double row0, double *col_out, double *row_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_centroids_launch(h, B, N, npix, nx, flux, mask, mask_stride, column0, row0, col_out, row_out,
                                     static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ quadratic centroids, difference images
int lk_cube_centroids_quadratic_batch_dev(lk_handle *h, int B, int N, int npix, int nx, const float *flux, const uint8_t *mask,
                                          int mask_stride, double column0, double row0, double *col_out, double *row_out,
                                          int32_t *peak_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_centroids_quadratic_launch(h, B, N, npix, nx, flux, mask, mask_stride, column0, row0, col_out, row_out,
                                               peak_out, static_cast<hipStream_t>(stream));
}

int lk_image_centroids_batch_dev(lk_handle *h, int B, int npix, int nx, const double *image, const uint8_t *mask, int mask_stride,
                                 double column0, double row0, int method, double *col_out, double *row_out, int32_t *peak_out,
                                 void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::image_centroids_launch(h, B, npix, nx, image, mask, mask_stride, column0, row0, method, col_out, row_out, peak_out,
                                      static_cast<hipStream_t>(stream));
}

int lk_cube_diffimage_batch_dev(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const float *flux_err,
                                const double *period, const double *transit_time, const double *duration, double in_width,
                                double out_inner, double out_outer, uint8_t *cadence_class, double *mean_in, double *mean_out,
                                double *diff, double *diff_err, int32_t *n_in, int32_t *n_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_diffimage_launch(h, B, N, npix, time, flux, flux_err, period, transit_time, duration, in_width, out_inner,
                                     out_outer, cadence_class, mean_in, mean_out, diff, diff_err, n_in, n_out,
                                     static_cast<hipStream_t>(stream));
}

int lk_diffimage_offsets_batch_dev(lk_handle *h, int B, const int32_t *n_in, const int32_t *n_out, const double *diff_col,
                                   const double *diff_row, const double *out_col, const double *out_row, double *offset,
                                   double *offset_pix, int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::centroid_offsets_launch(h, B, nullptr, n_in, n_out, diff_col, diff_row, out_col, out_row, offset, offset_pix, status,
                                       static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ background
int lk_cube_background_batch_dev(lk_handle *h, int B, int N, int npix, const float *cube, const uint8_t *mask, int mask_stride,
                                 int want_scatter, float *bkg, int32_t *n_pixels, float *scatter, float *cube_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_background_launch(h, B, N, npix, cube, mask, mask_stride, want_scatter, bkg, n_pixels, scatter, cube_out,
                                      static_cast<hipStream_t>(stream));
}

int lk_cube_subtract_rows_batch_dev(lk_handle *h, int B, int N, int npix, const float *cube, const float *rows, float *cube_out,
                                    void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_subtract_rows_launch(h, B, N, npix, cube, rows, cube_out, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ amplitude images
int lk_cube_ampimage_batch_dev(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const double *frequency,
                               int nterms, const double *t_ref, double *theta, double *level, double *amplitude, double *phase,
                               double *amplitude_err, double *snr, double *chi2, int32_t *n_used, int32_t *fit_status,
                               void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_ampimage_launch(h, B, N, npix, time, flux, frequency, nterms, t_ref, theta, level, amplitude, phase,
                                    amplitude_err, snr, chi2, n_used, fit_status, static_cast<hipStream_t>(stream));
}

int lk_ampimage_offsets_batch_dev(lk_handle *h, int B, const int32_t *fit_status, const double *amp_col, const double *amp_row,
                                  const double *level_col, const double *level_row, double *offset, double *offset_pix,
                                  int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::centroid_offsets_launch(h, B, fit_status, nullptr, nullptr, amp_col, amp_row, level_col, level_row, offset, offset_pix,
                                       status, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ pixel periodograms
int lk_cube_pixel_ls_batch_dev(lk_handle *h, int B, int N, int npix, const double *time, const float *flux, const double *frequency,
                               int F, int normalization, double oversample_factor, const double *t_ref, double *power,
                               double *peak_power, int32_t *peak_index, int32_t *n_used, int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_pixelpg_launch(h, B, N, npix, time, flux, frequency, F, normalization, oversample_factor, t_ref, power,
                                   peak_power, peak_index, n_used, status, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------ PSF photometry
int lk_cube_psf_photometry_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                                     const float *flux_err, const uint8_t *mask, int mask_stride, int S_max,
                                     const double *star_col, const double *star_row, const double *sigma, const double *shift_col,
                                     const double *shift_row, double column0, double row0, int use_flux_err, int32_t *star_off,
                                     double *time_out, double *flux_out, double *flux_err_out, double *background, double *chi2,
                                     int32_t *n_used, int8_t *cadence_status, int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_psfphot_launch(h, B, N, ny, nx, time, flux, flux_err, mask, mask_stride, S_max, star_col, star_row, sigma,
                                   shift_col, shift_row, column0, row0, use_flux_err, star_off, time_out, flux_out, flux_err_out, background,
                                   chi2, n_used, cadence_status, status, static_cast<hipStream_t>(stream));
}

int lk_cube_prf_photometry_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                                     const float *flux_err, const uint8_t *mask, int mask_stride, int S_max,
                                     const double *star_col, const double *star_row, const float *prf_table, int n_prf, int Ty,
                                     int Tx, int oversample, const int32_t *prf_index, const double *shift_col,
                                     const double *shift_row, double column0, double row0, int use_flux_err, int32_t *star_off,
                                     double *time_out, double *flux_out, double *flux_err_out, double *background, double *chi2,
                                     int32_t *n_used, int8_t *cadence_status, int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_prfphot_launch(h, B, N, ny, nx, time, flux, flux_err, mask, mask_stride, S_max, star_col, star_row, prf_table,
                                   n_prf, Ty, Tx, oversample, prf_index, shift_col, shift_row, column0, row0, use_flux_err, star_off,
                                   time_out, flux_out, flux_err_out, background, chi2, n_used, cadence_status, status,
                                   static_cast<hipStream_t>(stream));
}

int lk_cube_psf_fit_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                              const float *flux_err, const uint8_t *mask, int mask_stride, int S_max, const double *star_col,
                              const double *star_row, const double *sigma, const double *shift0_col, const double *shift0_row,
                              int max_iter, double tol, double max_step, double max_shift, double column0, double row0,
                              int use_flux_err, int32_t *star_off, double *time_out, double *flux_out, double *flux_err_out,
                              double *background, double *chi2, double *shift_col, double *shift_row, double *shift_col_err,
                              double *shift_row_err, double *last_step, int32_t *n_iter, int32_t *n_used, int8_t *cadence_status,
                              int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_psffit_launch(h, B, N, ny, nx, time, flux, flux_err, mask, mask_stride, S_max, star_col, star_row, sigma,
                                  shift0_col, shift0_row, max_iter, tol, max_step, max_shift, column0, row0, use_flux_err, star_off,
                                  time_out, flux_out, flux_err_out, background, chi2, shift_col, shift_row, shift_col_err,
                                  shift_row_err, last_step, n_iter, n_used, cadence_status, status, static_cast<hipStream_t>(stream));
}

int lk_cube_prf_fit_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                              const float *flux_err, const uint8_t *mask, int mask_stride, int S_max, const double *star_col,
                              const double *star_row, const float *prf_table, int n_prf, int Ty, int Tx, int oversample,
                              const int32_t *prf_index, const double *shift0_col, const double *shift0_row, int max_iter, double tol,
                              double max_step, double max_shift, double column0, double row0, int use_flux_err, int32_t *star_off,
                              double *time_out, double *flux_out, double *flux_err_out, double *background, double *chi2,
                              double *shift_col, double *shift_row, double *shift_col_err, double *shift_row_err, double *last_step,
                              int32_t *n_iter, int32_t *n_used, int8_t *cadence_status, int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_prffit_launch(h, B, N, ny, nx, time, flux, flux_err, mask, mask_stride, S_max, star_col, star_row, prf_table, n_prf,
                                  Ty, Tx, oversample, prf_index, shift0_col, shift0_row, max_iter, tol, max_step, max_shift, column0,
                                  row0, use_flux_err, star_off, time_out, flux_out, flux_err_out, background, chi2, shift_col, shift_row,
                                  shift_col_err, shift_row_err, last_step, n_iter, n_used, cadence_status, status,
                                  static_cast<hipStream_t>(stream));
}

int lk_cube_psf_width_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                                const float *flux_err, const uint8_t *mask, int mask_stride, int S_max, const double *star_col,
                                const double *star_row, const double *sigma0, const double *shift_col, const double *shift_row,
                                const uint8_t *cadence_mask, int max_iter, double tol, double max_step, double min_sigma,
                                double max_sigma, double column0, double row0, int use_flux_err, double *sigma, double *sigma_err,
                                double *sigma_cov, double *chi2, double *last_step, double *trace, int32_t *n_iter,
                                int32_t *n_cadences, int64_t *n_pixels, int8_t *cadence_status, int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_psfwidth_launch(h, B, N, ny, nx, time, flux, flux_err, mask, mask_stride, S_max, star_col, star_row, sigma0,
                                    shift_col, shift_row, cadence_mask, max_iter, tol, max_step, min_sigma, max_sigma, column0, row0,
                                    use_flux_err, sigma, sigma_err, sigma_cov, chi2, last_step, trace, n_iter, n_cadences, n_pixels,
                                    cadence_status, status, static_cast<hipStream_t>(stream));
}

int lk_cube_psf_positions_batch_dev(lk_handle *h, int B, int N, int ny, int nx, const double *time, const float *flux,
                                    const float *flux_err, const uint8_t *mask, int mask_stride, int S_max, const double *star_col,
                                    const double *star_row, const double *sigma, const uint8_t *fit_star, const double *shift_col,
                                    const double *shift_row, const uint8_t *cadence_mask, int max_iter, double tol, double max_step,
                                    double max_offset, double column0, double row0, int use_flux_err, double *star_col_out,
                                    double *star_row_out, double *star_col_err, double *star_row_err, double *position_cov,
                                    double *chi2, double *last_step, double *trace, int32_t *n_iter, int32_t *n_cadences,
                                    int64_t *n_pixels, int8_t *cadence_status, int32_t *status, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::cube_psfpos_launch(h, B, N, ny, nx, time, flux, flux_err, mask, mask_stride, S_max, star_col, star_row, sigma, fit_star,
                                  shift_col, shift_row, cadence_mask, max_iter, tol, max_step, max_offset, column0, row0, use_flux_err,
                                  star_col_out, star_row_out, star_col_err, star_row_err, position_cov, chi2, last_step, trace, n_iter,
                                  n_cadences, n_pixels, cadence_status, status, static_cast<hipStream_t>(stream));
}

int lk_sff_scratch_bytes(int B, const int64_t *n_off, const int32_t *n_knots, const int32_t *win_off, int bins, int degree,
                         int64_t max_scratch_bytes, int64_t *bytes, int *n_chunks) {
    return lk::sff_scratch_bytes(B, n_off, n_knots, win_off, bins, degree, max_scratch_bytes, bytes, n_chunks);
}

int lk_sff_arclength_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *centroid_col,
                               const double *centroid_row, double *arclength, int32_t *flipped, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::sff_arclength_launch(h, B, n_off_host, centroid_col, centroid_row, arclength, flipped,
                                    static_cast<hipStream_t>(stream));
}

int lk_sff_arclength_batch(lk_handle *h, int B, const int64_t *n_off, const double *centroid_col, const double *centroid_row,
                           double *arclength, int32_t *flipped) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 0 && n_off != nullptr, "bad batch description");
    if (B == 0 || n_off[B] == 0) return LK_OK;
    LK_REQUIRE(centroid_col && centroid_row && arclength, "NULL buffer");
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dc, *dr;
    double *da;
    int32_t *dfl;
    lk::StagedCall io(h);
    int rc = io.in(dc, centroid_col, ntot).in(dr, centroid_row, ntot).out(da, arclength, ntot).out(dfl, flipped, (size_t)B).stage();
    if (rc) return rc;
    rc = lk::sff_arclength_launch(h, B, n_off, dc, dr, da, dfl, nullptr);
    return rc ? rc : io.finish();
}

int lk_sff_design_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                            const double *flux_err, const double *arclength, const int32_t *win_off, const int32_t *window_points,
                            int bins, int degree, int n_knots, double *X, double *prior_mu, double *prior_sigma,
                            double *knots_time, double *knots_win, double *f_out, double *e_out, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::sff_design_launch(h, B, n_off_host, time, flux, flux_err, arclength, win_off, window_points, bins, degree, n_knots, X,
                                 prior_mu, prior_sigma, knots_time, knots_win, f_out, e_out, static_cast<hipStream_t>(stream));
}

int lk_sff_correct_batch_dev(lk_handle *h, int B, const int64_t *n_off_host, const double *time, const double *flux,
                             const double *flux_err, const double *centroid_col, const double *centroid_row,
                             const uint8_t *cadence_mask, const int32_t *win_off, const int32_t *window_points, int bins,
                             int degree, double timescale, int restore_trend, double clip_sigma, int niters, void *scratch,
                             int64_t scratch_bytes, double *flux_out, double *err_out, uint8_t *outlier, int32_t *status_host,
                             double *arclength, double *spline, double *sff, double *w, int w_pitch, void *stream) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_HIP_CHECK(hipSetDevice(h->device));
    return lk::sff_correct_launch(h, B, n_off_host, time, flux, flux_err, centroid_col, centroid_row, cadence_mask, win_off,
                                  window_points, bins, degree, timescale, restore_trend, clip_sigma, niters, scratch, scratch_bytes,
                                  flux_out, err_out, outlier, status_host, arclength, spline, sff, w, w_pitch,
                                  static_cast<hipStream_t>(stream));
}

int lk_sff_correct_batch(lk_handle *h, int B, const int64_t *n_off, const double *time, const double *flux, const double *flux_err,
                         const double *centroid_col, const double *centroid_row, const uint8_t *cadence_mask,
                         const int32_t *win_off, const int32_t *window_points, int bins, int degree, double timescale,
                         int restore_trend, double clip_sigma, int niters, int64_t max_scratch_bytes, double *flux_out,
                         double *err_out, uint8_t *outlier, int32_t *status, double *arclength, double *spline, double *sff,
                         double *w, int w_pitch) {
    LK_REQUIRE(h != nullptr, "handle is NULL");
    LK_REQUIRE(B >= 1 && n_off != nullptr && win_off != nullptr, "bad batch description");
    LK_REQUIRE(time && flux && flux_err && centroid_col && centroid_row && flux_out && err_out && outlier && status, "NULL buffer");
    LK_REQUIRE(timescale > 0.0, "timescale must be positive");
    LK_REQUIRE(!w || w_pitch >= 1, "w needs its row pitch");
    // the block is sized for the widths the times imply (the launcher derives the same widths from the device's copy; a target
    // it then finds non-finite is simply not fitted)
    std::vector<int32_t> nk((size_t)B);
    for (int b = 0; b < B; ++b) {
        LK_REQUIRE(n_off[b + 1] - n_off[b] >= 2, "target %d has fewer than 2 cadences", b);
        const double span = (time[n_off[b + 1] - 1] - time[n_off[b]]) / timescale;
        nk[b] = span >= 0.0 && span < 1e6 ? (int)span : 0;
    }
    int64_t bytes = 0;
    int rc = lk::sff_scratch_bytes(B, n_off, nk.data(), win_off, bins, degree, max_scratch_bytes, &bytes, nullptr);
    if (rc) return rc;
    LK_HIP_CHECK(hipSetDevice(h->device));
    const size_t ntot = (size_t)n_off[B];
    const double *dt, *df, *de, *dc, *dr;
    const uint8_t *dcm;
    double *dfo, *deo, *da, *dsp, *dsf, *dw;
    uint8_t *dout;
    char *dscr;
    lk::StagedCall io(h);
    rc = io.in(dt, time, ntot).in(df, flux, ntot).in(de, flux_err, ntot).in(dc, centroid_col, ntot).in(dr, centroid_row, ntot)
             .in(dcm, cadence_mask, ntot).out(dfo, flux_out, ntot).out(deo, err_out, ntot).out(dout, outlier, ntot)
             .out(da, arclength, ntot).out(dsp, spline, ntot).out(dsf, sff, ntot).out(dw, w, (size_t)B * (w ? w_pitch : 0))
             .scratch(dscr, (size_t)bytes).stage();
    if (rc) return rc;
    rc = lk::sff_correct_launch(h, B, n_off, dt, df, de, dc, dr, dcm, win_off, window_points, bins, degree, timescale, restore_trend,
                                clip_sigma, niters, dscr, bytes, dfo, deo, dout, status, da, dsp, dsf, dw, w_pitch, nullptr);
    return rc ? rc : io.finish();
}

}  // extern "C"
