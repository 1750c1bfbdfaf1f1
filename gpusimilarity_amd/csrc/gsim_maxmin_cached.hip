// gsim_maxmin_cached.hip -- the MaxMin pass kernels of gsim_maxmin.hip with default-policy table loads (launch_maxmin_pass_cached):
// for tables whose rows and state fit the 256 MiB Infinity Cache, which every pass then re-reads.
#define GSIM_STREAM_LOAD_DEFAULT_POLICY
#include "gsim_maxmin.hip"
