// rocfft_util.hpp -- what every rocFFT user of librmt shares (dct1.hip's fallback, periodic.hip,
// imex.hip): the status check, the one process-wide rocfft_setup, and the owner of a pair of
// plans with their execution info and work buffer.
#pragma once
#include "rmt_internal.hpp"

namespace rmt {

inline int rocfft_ok(rocfft_status s, const char *what) {
    if (s != rocfft_status_success) {
        set_error(std::string("rocFFT: ") + what + " failed (" + std::to_string((int)s) + ")");
        return RMT_EDEVICE;
    }
    return RMT_OK;
}

// rocfft_setup, once per process (before the first plan)
inline int rocfft_ready() {
    static bool ready = false;
    if (!ready) { RMT_TRY(rocfft_ok(rocfft_setup(), "setup")); ready = true; }
    return RMT_OK;
}

// Up to two plans that run one at a time, so they share an execution info and a work buffer
// of the larger size.  Create the plans into plan[], then finish(); on(stream) before a
// rocfft_execute(plan[k], .., info).
struct RocfftPlans {
    rocfft_plan plan[2] = {nullptr, nullptr};
    rocfft_execution_info info = nullptr;
    void *work = nullptr;
    size_t work_bytes = 0;

    RocfftPlans() = default;
    RocfftPlans(const RocfftPlans &) = delete;
    RocfftPlans &operator=(const RocfftPlans &) = delete;
    ~RocfftPlans() {
        for (rocfft_plan p : plan) if (p) rocfft_plan_destroy(p);
        if (info) rocfft_execution_info_destroy(info);
        (void)hipFree(work);
    }
    int finish() {
        size_t w[2] = {0, 0};
        for (int k = 0; k < 2; ++k)
            if (plan[k]) rocfft_plan_get_work_buffer_size(plan[k], &w[k]);
        work_bytes = std::max(w[0], w[1]);
        if (work_bytes) RMT_HIP(hipMalloc(&work, work_bytes));
        RMT_TRY(rocfft_ok(rocfft_execution_info_create(&info), "execution_info_create"));
        if (work_bytes)
            RMT_TRY(rocfft_ok(rocfft_execution_info_set_work_buffer(info, work, work_bytes),
                              "set_work_buffer"));
        return RMT_OK;
    }
    int on(hipStream_t st) {
        return rocfft_ok(rocfft_execution_info_set_stream(info, st), "set_stream");
    }
};

}  // namespace rmt
