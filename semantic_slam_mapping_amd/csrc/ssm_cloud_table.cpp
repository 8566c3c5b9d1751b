// ssm_cloud_table.cpp -- the host's half of the cloud-segment table (cloud_table.h): the numbering of a call's points and each block's first
// cloud, and the count of a call's points against its stage's bound.  Index arithmetic only, in 64 bits: plain C++ that host/test_cloud_table.cpp runs under the
// CPU sanitizers.
#include "ssm_host.h"

int64_t cloud_table_build(CloudSeg* seg, int m, int T, int32_t* blk, int64_t* blocks)
{
    int64_t at = 0;
    for (int k = 0; k < m; k++) { seg[k].off = at; at += seg[k].n; }
    *blocks = (at + T - 1) / T;
    // a block's first point b T is below the total, so the walk ends inside seg; an empty cloud (off + n == the next cloud's off) is stepped over
    if (blk) for (int64_t b = 0, k = 0; b < *blocks; b++) { while (b * T >= seg[k].off + seg[k].n) k++; blk[b] = (int32_t)k; }
    return at;
}
bool cloud_count(const int32_t* n, int m, int stride, int64_t* total)
{
    *total = 0;
    for (int k = 0; k < m; k++) { if (n[k] < 0) return false; *total += ((int64_t)n[k] + stride - 1) / stride; }
    return true;
}
int cloud_bound_check(ssm_ctx* c, const CloudRule& R, int64_t total)
{
    if (R.sums ? !ssm_alignc::sums_fit(*R.sums, total) : total >= R.limit) return host_fail(c, SSM_E_INVAL, R.bound_msg);
    return SSM_OK;
}
int cloud_total_check(ssm_ctx* c, const CloudRule& R, const int32_t* n, int m, int64_t* total)
{
    if (!cloud_count(n, m, R.stride, total)) return host_fail(c, SSM_E_INVAL, R.negative_msg);
    return cloud_bound_check(c, R, *total);
}
