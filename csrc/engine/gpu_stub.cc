// Linked into CPU-only builds (no HIP engine object).
#include <stdexcept>

#include "engine.h"
#include "lane_check.h"
#include "icnt_sweep.h"

namespace asim {
std::unique_ptr<Engine> make_gpu_engine() { return nullptr; }
bool gpu_engine_available() { return false; }
}  // namespace asim

namespace asim {
int gpu_cu_count() { return 0; }
int gpu_cus_per_sim(uint32_t n_sm, uint32_t n_mem) { return (int)(n_sm + n_mem); }
std::map<std::string, uint64_t> gpu_pool_stats() { return {}; }
void gpu_pool_trim() {}
void* gpu_pool_alloc(size_t) { throw std::runtime_error("no GPU engine in this build"); }
void gpu_pool_release(void*) {}
std::map<std::string, uint64_t> gpu_batch_stats() { return {}; }
std::map<std::string, std::map<std::string, uint64_t>> gpu_engine_modes() { return {}; }
EngineKernelInfo gpu_engine_kernel_info() { return EngineKernelInfo{}; }
}  // namespace asim

namespace asim {
bool gpu_coalesce_kernel(const HostKernel&, const SimCfg&, int, ReadyKernel&, IngestStats*) { return false; }
}  // namespace asim

namespace asim {
int gpu_current_device() { return -1; }
}  // namespace asim

namespace asim {
// no device: the SeqPar half only (ran stays false)
LaneCheckResult lane_policy_check(const std::string& name, int n, const std::vector<uint64_t>& values,
                                  const std::vector<uint64_t>& mask) {
  LaneCheckResult r;
  lane_check_host(lane_plan(name, n, values, mask), n, values, mask, r);
  return r;
}
}  // namespace asim

namespace asim {
// no device: the batch entry point refuses engine "gpu" before it gets here
uint64_t icnt_sweep_budget_bytes(uint64_t) { throw std::runtime_error("no GPU engine in this build"); }
bool icnt_sweep_run_chunk(const OpenLoopNet&, const std::vector<OpenLoopPoint>&, uint64_t, bool,
                          std::vector<OpenLoopRaw>&) {
  throw std::runtime_error("no GPU engine in this build");
}
std::map<std::string, uint64_t> icnt_sweep_kernel_info() { return {}; }
bool icnt_rr_run_chunk(const OpenLoopNet&, const std::vector<RrUnit>&, uint64_t, bool, std::vector<RrRaw>&) {
  throw std::runtime_error("no GPU engine in this build");
}
std::map<std::string, uint64_t> icnt_rr_kernel_info() { return {}; }
bool icnt_net_run_chunk(const NetList&, const std::vector<NetUnit>&, uint64_t, bool, std::vector<OpenLoopRaw>&) {
  throw std::runtime_error("no GPU engine in this build");
}
std::map<std::string, uint64_t> icnt_net_kernel_info() { return {}; }
bool icnt_cl_run_chunk(const OpenLoopNet&, const std::vector<ClUnit>&, uint64_t, bool, std::vector<ClRaw>&) {
  throw std::runtime_error("no GPU engine in this build");
}
std::map<std::string, uint64_t> icnt_cl_kernel_info() { return {}; }
bool icnt_cln_run_chunk(const ClList&, const std::vector<ClnUnit>&, uint64_t, bool, std::vector<ClRaw>&) {
  throw std::runtime_error("no GPU engine in this build");
}
std::map<std::string, uint64_t> icnt_cln_kernel_info() { return {}; }
}  // namespace asim
