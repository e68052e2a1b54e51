// fi_robust.h -- robust fits: data points reweighted by their residuals (fi_robust.hip), behind the C ABI (fi_capi.hip).
#pragma once

#include "fi_internal.h"

namespace fi {

// what one reweighting step found (fi_robust_stats carries it to the caller)
struct RobustStep {
	float scale = 0.0f;
	float max_weight_change = 0.0f;
	long  points_used = 0, points_zeroed = 0;
};

// FI_ERR_UNSUPPORTED / FI_ERR_STATE where the contract says so (include/fi_hip.h); returns the number of data points
long robust_check(const fi_ctx* c);
long robust_point_count(const fi_ctx* c);
// field: the owned values (fp32, `memory`) or nullptr for the last solution where it lives; residuals: float[n], `memory`
void robust_residuals(fi_ctx* c, const float* field, float* residuals, int memory);
// one step; the rows are emitted again unless the scale is 0.  omega: float[n] (`memory`) or nullptr
RobustStep robust_reweight(fi_ctx* c, const float* field, int loss, float tuning, float scale, float* omega, int memory);
void robust_reset(fi_ctx* c);

}  // namespace fi
