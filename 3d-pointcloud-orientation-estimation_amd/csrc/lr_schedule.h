// lr_schedule.h -- the learning-rate schedule of the scheduled optimiser as ONE function, compiled for the host (pnpp_lr_factor) and for
// the device (adamw_sched_kernel's thread 0): what the host reports for a step count is what a captured launch applies at that count.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/pnpp_hip.h"

namespace pnpp {

// The factor f the base rate is multiplied by at the update that follows `s` completed ones (torch's scheduler epoch), float64:
//   s < warmup                 f = start + (1 - start) * s / warmup                        (LinearLR(start_factor, total_iters = warmup))
//   constant                   f = 1
//   cosine, u = (s - warmup) / (total - warmup)
//                              f = min + (1 - min) * (1 + cos(pi u)) / 2,  f = min for s >= total   (CosineAnnealingLR, closed form)
//   step                       f = max(min, gamma ^ floor((s - warmup) / every))           (StepLR, floored at min)
// The descriptor has passed check_schedule (optim_sched_kernels.hip): total > warmup for cosine, every > 0 for step.
__host__ __device__ inline double lr_schedule_factor(const pnpp_optim_desc &d, uint64_t s) {
    if (s < d.warmup) return d.start_factor + (1.0 - d.start_factor) * ((double)s / (double)d.warmup);
    if (d.sched_kind == PNPP_SCHED_COSINE) {
        if (s >= d.total) return d.min_factor;
        const double u = (double)(s - d.warmup) / (double)(d.total - d.warmup);
        return d.min_factor + (1.0 - d.min_factor) * (0.5 * (1.0 + cos(3.14159265358979323846 * u)));
    }
    if (d.sched_kind == PNPP_SCHED_STEP) {
        const double f = pow(d.gamma, (double)((s - d.warmup) / d.every));
        return f > d.min_factor ? f : d.min_factor;
    }
    return 1.0;
}

}  // namespace pnpp
