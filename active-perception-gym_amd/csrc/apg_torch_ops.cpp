// apg_torch_ops.cpp — PyTorch custom ops (TORCH_LIBRARY(apgym, ...)) over the C ABI of libapgym_hip.so.
//
// The envs' hot path calls these instead of marshalling the C-ABI structs through ctypes on every
// step: an env handle (torch.classes.apgym.LidarEnv / ImageEnv) is built once from the env's config
// fields and its persistent device buffers, and the ops launch on PyTorch's current HIP stream, so
// they are stream-ordered with the caller's tensors and can be captured into a torch.cuda.CUDAGraph
// (hipGraph) like any ATen op.
//
//   torch.ops.apgym.lidar_reset(LidarEnv env, int seed, bool use_seed) -> ()
//   torch.ops.apgym.lidar_step(LidarEnv env, Tensor action, Tensor prediction) -> ()
//   torch.ops.apgym.image_reset(ImageEnv env) -> ()
//   torch.ops.apgym.image_step(ImageEnv env, Tensor action, Tensor prediction, int t, int prev_done) -> ()
//   torch.ops.apgym.unpack_map_bits(Tensor bits, int width, Tensor? env_ids, Tensor out, float wall, Tensor? err) -> ()
//   torch.ops.apgym.lidar_scan_poses(Tensor bits, int width, Tensor poses, Tensor? map_ids, Tensor beam_dirs,
//                                    float lidar_range, bool normalize, Tensor? observed, Tensor? scan, Tensor? score,
//                                    Tensor? err) -> ()
//   torch.ops.apgym.lidar_move_poses(Tensor bits, int width, Tensor poses, Tensor actions, Tensor? map_ids,
//                                    Tensor? max_steps, Tensor? origin, Tensor? origin_alias, Tensor pos, Tensor steps,
//                                    Tensor terminated, Tensor? base_reward, Tensor? odometry, Tensor? err) -> ()
//   torch.ops.apgym.lidar_pf_resample(Tensor poses, Tensor? logw, Tensor? score, Tensor? u, float score_scale,
//                                     float ess_frac, Tensor? weight, Tensor? estimate, Tensor? ess, Tensor? index,
//                                     Tensor? poses_out, Tensor? logw_out, Tensor? resampled, Tensor? err) -> ()
//   torch.ops.apgym.image_glimpse_scores(Tensor pool, int[] geo, float sensor_scale, Tensor index, Tensor positions,
//                                        Tensor? observed, Tensor? score, Tensor? glimpse, Tensor? err) -> ()
//   torch.ops.apgym.image_move(Tensor start, Tensor actions, float msl0, float msl1, int max_steps, Tensor pos,
//                              Tensor glimpse_pos, Tensor base_reward, Tensor? err) -> ()
//   torch.ops.apgym.image_overlap_scores(Tensor glimpse, Tensor glimpse_pos, Tensor target_glimpse, Tensor hypotheses,
//                                        int[] image_size, float sensor_scale, Tensor? logw, float gain, float tau,
//                                        Tensor sse, Tensor count, Tensor? logw_out, Tensor? err) -> ()
//
// Replaces, like the C ABI below it (include/apgym_capi.h): SyncVectorEnv.reset/step over
// TimeLimit(LIDARLocalization2DEnv) (ap_gym/envs/lidar_localization2d.py:293-389) and
// Image{Classification,Localization}VectorEnv reset/step (ap_gym/envs/image_classification.py:107-151,
// image_localization.py:131-181, image/image_perception_module.py:105-251).
// Build: hipcc (host code only) against torch's headers, linked to libapgym_hip.so (build.py).
#include <ATen/Tensor.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/custom_class.h>
#include <torch/library.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/apgym_capi.h"

namespace {

void *ptr(const at::Tensor &t) { return t.defined() && t.numel() > 0 ? t.data_ptr() : nullptr; }

void check(int rc, const char *what) {
  TORCH_CHECK(rc == APG_OK, what, " failed (", rc, "): ", apg_last_error());
}

apg_stream_t stream_of(const at::Device &d) { return (apg_stream_t)c10::hip::getCurrentHIPStream(d.index()).stream(); }

void check_io(const at::Tensor &t, const at::Device &d, int64_t numel, const char *name) {
  TORCH_CHECK(t.device() == d, name, " must be on ", d, ", got ", t.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() == numel, name, " must have ", numel, " elements, got ", t.numel());
}

// Buffers are passed in the C struct's field order; a 0-element tensor stands for NULL.  The handle
// keeps them alive for its lifetime.
template <class S>
void fill_ptrs(S &s, const std::vector<at::Tensor> &ts, const char *what) {
  constexpr size_t n = sizeof(S) / sizeof(void *);
  static_assert(sizeof(S) == n * sizeof(void *), "pointer-only struct");
  TORCH_CHECK(ts.size() == n, what, ": expected ", n, " buffers, got ", ts.size());
  void *p[n];
  for (size_t i = 0; i < n; i++) p[i] = ptr(ts[i]);
  std::memcpy(&s, p, sizeof(S));
}

struct LidarEnv : torch::CustomClassHolder {
  apg_lidar_config cfg{};
  apg_lidar_state st{};
  apg_lidar_outputs out{};
  std::vector<at::Tensor> keep;
  at::Device dev = at::Device(at::kCUDA, 0);

  // ints: num_envs, height, width, map_kind, is_static, static_map_index, beams, step_limit, max_rooms,
  // door_width, log_stats, sparse, out_row_bytes, prefetcher handle (apg_lidar_prefetcher_create's pointer or 0:
  // owned by the Python env), pool_len, stream_len; reals: lidar_range, loss_scale, loss_offset, branching_prob.  The state
  // buffers are the struct's fields in order: ..., the prefetch buffer, a 0-element placeholder for the prefetcher
  // field, the map pool (pool_occ, pool_free: 0-element tensors for the procedural kinds).
  LidarEnv(std::vector<int64_t> ints, std::vector<double> reals, std::vector<at::Tensor> state,
           std::vector<at::Tensor> outputs) {
    TORCH_CHECK(ints.size() == 16 && reals.size() == 4, "LidarEnv: 16 ints and 4 reals expected");
    cfg.num_envs = (int32_t)ints[0];
    cfg.height = (int32_t)ints[1];
    cfg.width = (int32_t)ints[2];
    cfg.map_kind = (int32_t)ints[3];
    cfg.is_static = (int32_t)ints[4];
    cfg.static_map_index = (int32_t)ints[5];
    cfg.beams = (int32_t)ints[6];
    cfg.step_limit = (int32_t)ints[7];
    cfg.max_rooms = (int32_t)ints[8];
    cfg.door_width = (int32_t)ints[9];
    cfg.log_stats = (int32_t)ints[10];
    cfg.sparse = (int32_t)ints[11];
    cfg.out_row_bytes = (int32_t)ints[12];
    cfg.pool_len = (int32_t)ints[14];
    cfg.stream_len = ints[15];
    cfg.lidar_range = (float)reals[0];
    cfg.loss_scale = (float)reals[1];
    cfg.loss_offset = (float)reals[2];
    cfg.branching_prob = reals[3];
    fill_ptrs(st, state, "LidarEnv state");
    fill_ptrs(out, outputs, "LidarEnv outputs");
    st.prefetcher = reinterpret_cast<void *>(static_cast<uintptr_t>(ints[13]));
    for (auto &t : state)
      if (t.defined() && t.numel() > 0) dev = t.device();
    keep = state;
    keep.insert(keep.end(), outputs.begin(), outputs.end());
  }
};

struct ImageEnv : torch::CustomClassHolder {
  apg_image_config cfg{};
  apg_image_state st{};
  apg_image_outputs out{};
  std::vector<at::Tensor> keep;
  at::Device dev = at::Device(at::kCUDA, 0);

  // ints: the 16 int32 fields of apg_image_config up to env_offset, pool_len, log_stats, sparse, out_row_bytes;
  // reals: sensor_scale, max_step[2], cell[2], ce_scale, ce_offset, mse_scale, mse_offset
  ImageEnv(std::vector<int64_t> ints, std::vector<double> reals, std::vector<at::Tensor> state,
           std::vector<at::Tensor> outputs) {
    TORCH_CHECK(ints.size() == 20 && reals.size() == 9, "ImageEnv: 20 ints and 9 reals expected");
    int32_t *f = &cfg.num_envs;  // num_envs .. env_offset: 16 consecutive int32 fields
    for (int i = 0; i < 16; i++) f[i] = (int32_t)ints[i];
    cfg.pool_len = ints[16];
    cfg.log_stats = (int32_t)ints[17];
    cfg.sparse = (int32_t)ints[18];
    cfg.out_row_bytes = (int32_t)ints[19];
    cfg.sensor_scale = reals[0];
    cfg.max_step[0] = reals[1];
    cfg.max_step[1] = reals[2];
    cfg.cell[0] = reals[3];
    cfg.cell[1] = reals[4];
    cfg.ce_scale = reals[5];
    cfg.ce_offset = reals[6];
    cfg.mse_scale = (float)reals[7];
    cfg.mse_offset = (float)reals[8];
    fill_ptrs(st, state, "ImageEnv state");
    fill_ptrs(out, outputs, "ImageEnv outputs");
    for (auto &t : state)
      if (t.defined() && t.numel() > 0) dev = t.device();
    keep = state;
    keep.insert(keep.end(), outputs.begin(), outputs.end());
  }
};
static_assert(offsetof(apg_image_config, env_offset) == 15 * sizeof(int32_t), "apg_image_config int32 prefix");

void lidar_reset(const c10::intrusive_ptr<LidarEnv> &e, int64_t seed, bool use_seed) {
  const c10::DeviceGuard guard(e->dev);
  check(apg_lidar_reset(&e->cfg, &e->st, (uint64_t)seed, use_seed ? 1 : 0, &e->out, stream_of(e->dev)),
        "apg_lidar_reset");
}

void lidar_step(const c10::intrusive_ptr<LidarEnv> &e, const at::Tensor &action, const at::Tensor &prediction) {
  const c10::DeviceGuard guard(e->dev);
  const int64_t n2 = 2 * (int64_t)e->cfg.num_envs;
  check_io(action, e->dev, n2, "action");
  check_io(prediction, e->dev, n2, "prediction");
  check(apg_lidar_step(&e->cfg, &e->st, action.data_ptr<float>(), prediction.data_ptr<float>(), &e->out,
                       stream_of(e->dev)),
        "apg_lidar_step");
}

void image_reset(const c10::intrusive_ptr<ImageEnv> &e) {
  const c10::DeviceGuard guard(e->dev);
  check(apg_image_reset(&e->cfg, &e->st, &e->out, stream_of(e->dev)), "apg_image_reset");
}

// prev_done: bit 0 the previous step terminated the batch, bit 1 its draws were made ahead (apg_image_step)
void image_step(const c10::intrusive_ptr<ImageEnv> &e, const at::Tensor &action, const at::Tensor &prediction,
                int64_t t, int64_t prev_done) {
  const c10::DeviceGuard guard(e->dev);
  const int64_t n = e->cfg.num_envs;
  check_io(action, e->dev, 2 * n, "action");
  const int64_t pw = e->cfg.kind == APG_IMAGE_CLASSIFY ? (int64_t)e->cfg.num_classes : 2;
  check_io(prediction, e->dev, pw * n, "prediction");
  check(apg_image_step(&e->cfg, &e->st, action.data_ptr<float>(), prediction.data_ptr<float>(), (int32_t)t,
                       (int32_t)prev_done, &e->out, stream_of(e->dev)),
        "apg_image_step");
}

// bits: int64 [n_src, H, ceil(width / 64)] occupancy rows (apg_lidar_state.occ's layout); out: the [M, H, width(, 1)]
// maps in its own dtype (float32 / float16 / bfloat16 / uint8), M = len(env_ids) or n_src; err: the int32 [1] error word
// a bad id is flagged in (APG_ERR_INDEX), or None
void unpack_map_bits(const at::Tensor &bits, int64_t width, const c10::optional<at::Tensor> &env_ids, at::Tensor out,
                     double wall, const c10::optional<at::Tensor> &err) {
  TORCH_CHECK(bits.is_cuda(), "bits must be on a GPU device, got ", bits.device());
  const at::Device dev = bits.device();
  const c10::DeviceGuard guard(dev);
  TORCH_CHECK(bits.scalar_type() == at::kLong && bits.dim() == 3 && bits.is_contiguous(),
              "bits must be a contiguous int64 [n_src, H, ceil(width / 64)] tensor");
  TORCH_CHECK(width >= 1 && width <= 511 && bits.size(2) == (width + 63) / 64, "bits has ", bits.size(2),
              " words per row, width ", width, " needs ", (width + 63) / 64, " (width 1..511)");
  const int64_t n_src = bits.size(0), h = bits.size(1);
  TORCH_CHECK(h >= 1 && h <= 511, "map height must be 1..511, got ", h);
  int64_t count = n_src;
  const int64_t *ids = nullptr;
  if (env_ids.has_value() && env_ids->defined()) {
    TORCH_CHECK(env_ids->device() == dev && env_ids->scalar_type() == at::kLong && env_ids->dim() == 1 &&
                    env_ids->is_contiguous(),
                "env_ids must be a contiguous 1-d int64 tensor on ", dev);
    count = env_ids->numel();
    ids = count ? env_ids->data_ptr<int64_t>() : nullptr;
  }
  TORCH_CHECK(out.device() == dev && out.is_contiguous(), "out must be a contiguous tensor on ", dev);
  TORCH_CHECK(out.numel() == count * h * width, "out must have ", count * h * width, " elements, got ", out.numel());
  int dtype;
  switch (out.scalar_type()) {
    case at::kFloat: dtype = APG_UNPACK_F32; break;
    case at::kHalf: dtype = APG_UNPACK_F16; break;
    case at::kBFloat16: dtype = APG_UNPACK_BF16; break;
    case at::kByte: dtype = APG_UNPACK_U8; break;
    default: TORCH_CHECK(false, "out must be float32, float16, bfloat16 or uint8, got ", out.scalar_type());
  }
  uint32_t *errp = nullptr;
  if (err.has_value() && err->defined()) {
    TORCH_CHECK(err->device() == dev && err->scalar_type() == at::kInt && err->numel() == 1,
                "err must be an int32 [1] tensor on ", dev);
    errp = reinterpret_cast<uint32_t *>(err->data_ptr());
  }
  check(apg_lidar_unpack_maps(reinterpret_cast<const uint64_t *>(ptr(bits)), n_src, (int)h, (int)width, ids, count, dtype,
                              (float)wall, ptr(out), errp, stream_of(dev)),
        "apg_lidar_unpack_maps");
}

// Exact scans and fused scores at caller-chosen poses (apg_lidar_scan_poses).  bits: int64 [n_src, H, ceil(width / 64)];
// poses: float32 [M, K, 2]; map_ids: int64 [M] or None; beam_dirs: float32 [B, 2]; observed: float32 [M, B] or None
// (needed with score); scan: float32 [M, K, B] or None; score: float32 [M, K] or None; err: int32 [1] or None.
void lidar_scan_poses(const at::Tensor &bits, int64_t width, const at::Tensor &poses,
                      const c10::optional<at::Tensor> &map_ids, const at::Tensor &beam_dirs, double lidar_range,
                      bool normalize, const c10::optional<at::Tensor> &observed, const c10::optional<at::Tensor> &scan,
                      const c10::optional<at::Tensor> &score, const c10::optional<at::Tensor> &err) {
  TORCH_CHECK(bits.is_cuda(), "bits must be on a GPU device, got ", bits.device());
  const at::Device dev = bits.device();
  const c10::DeviceGuard guard(dev);
  TORCH_CHECK(bits.scalar_type() == at::kLong && bits.dim() == 3 && bits.is_contiguous(),
              "bits must be a contiguous int64 [n_src, H, ceil(width / 64)] tensor");
  TORCH_CHECK(width >= 1 && width <= 511 && bits.size(2) == (width + 63) / 64, "bits has ", bits.size(2),
              " words per row, width ", width, " needs ", (width + 63) / 64, " (width 1..511)");
  TORCH_CHECK(poses.dim() == 3 && poses.size(2) == 2, "poses must be [M, K, 2]");
  const int64_t m = poses.size(0), k = poses.size(1);
  TORCH_CHECK(k <= INT32_MAX, "poses: too many poses per set");
  check_io(poses, dev, 2 * m * k, "poses");
  TORCH_CHECK(beam_dirs.dim() == 2 && beam_dirs.size(1) == 2, "beam_dirs must be [B, 2]");
  const int64_t b = beam_dirs.size(0);
  check_io(beam_dirs, dev, 2 * b, "beam_dirs");
  apg_scan_poses_args a{};
  a.occ = reinterpret_cast<const uint64_t *>(ptr(bits));
  a.poses = reinterpret_cast<const float *>(ptr(poses));
  a.beam_dirs = reinterpret_cast<const float *>(ptr(beam_dirs));
  if (map_ids.has_value() && map_ids->defined()) {
    TORCH_CHECK(map_ids->device() == dev && map_ids->scalar_type() == at::kLong && map_ids->dim() == 1 &&
                    map_ids->is_contiguous() && map_ids->numel() == m,
                "map_ids must be a contiguous int64 [M] tensor on ", dev);
    a.map_ids = reinterpret_cast<const int64_t *>(ptr(*map_ids));
  }
  if (observed.has_value() && observed->defined()) {
    check_io(*observed, dev, m * b, "observed");
    a.observed = reinterpret_cast<const float *>(ptr(*observed));
  }
  if (scan.has_value() && scan->defined()) {
    check_io(*scan, dev, m * k * b, "scan");
    a.scan = reinterpret_cast<float *>(ptr(*scan));
  }
  if (score.has_value() && score->defined()) {
    check_io(*score, dev, m * k, "score");
    TORCH_CHECK(a.observed || m * b == 0, "score needs observed");
    a.score = reinterpret_cast<float *>(ptr(*score));
  }
  if (err.has_value() && err->defined()) {
    TORCH_CHECK(err->device() == dev && err->scalar_type() == at::kInt && err->numel() == 1,
                "err must be an int32 [1] tensor on ", dev);
    a.err = reinterpret_cast<uint32_t *>(err->data_ptr());
  }
  a.n_src = bits.size(0);
  a.m = m;
  a.height = (int32_t)bits.size(1);
  a.width = (int32_t)width;
  a.k = (int32_t)k;
  a.beams = (int32_t)std::min<int64_t>(b, INT32_MAX);
  a.normalize = normalize ? 1 : 0;
  a.lidar_range = (float)lidar_range;
  check(apg_lidar_scan_poses(&a, stream_of(dev)), "apg_lidar_scan_poses");
}

// Open-loop rollouts of candidate actions from caller-chosen poses (apg_lidar_move_poses).  bits: int64
// [n_src, H, ceil(width / 64)]; poses: float32 [M, K, 2]; actions: float32 [M, K, T, 2]; map_ids: int64 [M] or None;
// max_steps: int32 [M] or None; origin: float32 [M, 2] or None; origin_alias: uint8 [M] or None; pos: float32
// [M, K, T, 2]; steps: int32 [M, K]; terminated: uint8 [M, K]; base_reward: float32 [M, K, T] or None; odometry:
// float32 [M, K, T, 2] or None (needs origin); err: int32 [1] or None.
void lidar_move_poses(const at::Tensor &bits, int64_t width, const at::Tensor &poses, const at::Tensor &actions,
                      const c10::optional<at::Tensor> &map_ids, const c10::optional<at::Tensor> &max_steps,
                      const c10::optional<at::Tensor> &origin, const c10::optional<at::Tensor> &origin_alias,
                      at::Tensor pos, at::Tensor steps, at::Tensor terminated,
                      const c10::optional<at::Tensor> &base_reward, const c10::optional<at::Tensor> &odometry,
                      const c10::optional<at::Tensor> &err) {
  TORCH_CHECK(bits.is_cuda(), "bits must be on a GPU device, got ", bits.device());
  const at::Device dev = bits.device();
  const c10::DeviceGuard guard(dev);
  TORCH_CHECK(bits.scalar_type() == at::kLong && bits.dim() == 3 && bits.is_contiguous(),
              "bits must be a contiguous int64 [n_src, H, ceil(width / 64)] tensor");
  TORCH_CHECK(width >= 1 && width <= 511 && bits.size(2) == (width + 63) / 64, "bits has ", bits.size(2),
              " words per row, width ", width, " needs ", (width + 63) / 64, " (width 1..511)");
  TORCH_CHECK(poses.dim() == 3 && poses.size(2) == 2, "poses must be [M, K, 2]");
  const int64_t m = poses.size(0), k = poses.size(1);
  TORCH_CHECK(k <= INT32_MAX, "poses: too many candidates per set");
  check_io(poses, dev, 2 * m * k, "poses");
  TORCH_CHECK(actions.dim() == 4 && actions.size(0) == m && actions.size(1) == k && actions.size(3) == 2,
              "actions must be [M, K, T, 2]");
  const int64_t t = actions.size(2);
  TORCH_CHECK(t >= 1 && t <= 4096, "actions: T must be in [1, 4096], got ", t);
  check_io(actions, dev, 2 * m * k * t, "actions");
  auto typed = [&](const at::Tensor &x, at::ScalarType st, int64_t numel, const char *name) {
    TORCH_CHECK(x.device() == dev && x.scalar_type() == st && x.is_contiguous() && x.numel() == numel, name,
                " must be a contiguous ", st, " tensor of ", numel, " elements on ", dev);
  };
  apg_move_poses_args a{};
  a.occ = reinterpret_cast<const uint64_t *>(ptr(bits));
  a.poses = reinterpret_cast<const float *>(ptr(poses));
  a.actions = reinterpret_cast<const float *>(ptr(actions));
  if (map_ids.has_value() && map_ids->defined()) {
    TORCH_CHECK(map_ids->dim() == 1, "map_ids must be 1-d");
    typed(*map_ids, at::kLong, m, "map_ids");
    a.map_ids = reinterpret_cast<const int64_t *>(ptr(*map_ids));
  }
  if (max_steps.has_value() && max_steps->defined()) {
    typed(*max_steps, at::kInt, m, "max_steps");
    a.max_steps = reinterpret_cast<const int32_t *>(ptr(*max_steps));
  }
  const bool has_origin = origin.has_value() && origin->defined();
  if (has_origin) {
    check_io(*origin, dev, 2 * m, "origin");
    a.origin = reinterpret_cast<const float *>(ptr(*origin));
  }
  if (origin_alias.has_value() && origin_alias->defined()) {
    TORCH_CHECK(has_origin, "origin_alias needs origin");
    typed(*origin_alias, at::kByte, m, "origin_alias");
    a.origin_alias = reinterpret_cast<const uint8_t *>(ptr(*origin_alias));
  }
  check_io(pos, dev, 2 * m * k * t, "pos");
  typed(steps, at::kInt, m * k, "steps");
  typed(terminated, at::kByte, m * k, "terminated");
  a.pos = reinterpret_cast<float *>(ptr(pos));
  a.steps = reinterpret_cast<int32_t *>(ptr(steps));
  a.terminated = reinterpret_cast<uint8_t *>(ptr(terminated));
  if (base_reward.has_value() && base_reward->defined()) {
    check_io(*base_reward, dev, m * k * t, "base_reward");
    a.base_reward = reinterpret_cast<float *>(ptr(*base_reward));
  }
  if (odometry.has_value() && odometry->defined()) {
    TORCH_CHECK(has_origin, "odometry needs origin");
    check_io(*odometry, dev, 2 * m * k * t, "odometry");
    a.odometry = reinterpret_cast<float *>(ptr(*odometry));
  }
  if (err.has_value() && err->defined()) {
    TORCH_CHECK(err->device() == dev && err->scalar_type() == at::kInt && err->numel() == 1,
                "err must be an int32 [1] tensor on ", dev);
    a.err = reinterpret_cast<uint32_t *>(err->data_ptr());
  }
  a.n_src = bits.size(0);
  a.m = m;
  a.height = (int32_t)bits.size(1);
  a.width = (int32_t)width;
  a.k = (int32_t)k;
  a.t = (int32_t)t;
  check(apg_lidar_move_poses(&a, stream_of(dev)), "apg_lidar_move_poses");
}

// Particle weights, estimate, ESS and systematic resampling (apg_lidar_pf_resample).  poses: float32 [M, K, 2]; logw,
// score: float32 [M, K] or None; u: float32 [M] or None (ess_frac <= 0); weight, logw_out: float32 [M, K]; estimate:
// float32 [M, 2]; ess: float32 [M]; index: int32 [M, K]; poses_out: float32 [M, K, 2]; resampled: uint8 [M]; err:
// int32 [1]; every output or None.  logw_out may be logw itself.
void lidar_pf_resample(const at::Tensor &poses, const c10::optional<at::Tensor> &logw,
                       const c10::optional<at::Tensor> &score, const c10::optional<at::Tensor> &u, double score_scale,
                       double ess_frac, const c10::optional<at::Tensor> &weight,
                       const c10::optional<at::Tensor> &estimate, const c10::optional<at::Tensor> &ess,
                       const c10::optional<at::Tensor> &index, const c10::optional<at::Tensor> &poses_out,
                       const c10::optional<at::Tensor> &logw_out, const c10::optional<at::Tensor> &resampled,
                       const c10::optional<at::Tensor> &err) {
  TORCH_CHECK(poses.is_cuda(), "poses must be on a GPU device, got ", poses.device());
  const at::Device dev = poses.device();
  const c10::DeviceGuard guard(dev);
  TORCH_CHECK(poses.dim() == 3 && poses.size(2) == 2, "poses must be [M, K, 2]");
  const int64_t m = poses.size(0), k = poses.size(1);
  TORCH_CHECK(k >= 1 && k <= 4096, "poses: K must be in 1..4096, got ", k);
  check_io(poses, dev, 2 * m * k, "poses");
  apg_pf_resample_args a{};
  a.poses = reinterpret_cast<const float *>(ptr(poses));
  auto f32 = [&](const c10::optional<at::Tensor> &x, int64_t numel, const char *name) -> float * {
    if (!x.has_value() || !x->defined()) return nullptr;
    check_io(*x, dev, numel, name);
    return reinterpret_cast<float *>(ptr(*x));
  };
  auto typed = [&](const c10::optional<at::Tensor> &x, at::ScalarType st, int64_t numel, const char *name) -> void * {
    if (!x.has_value() || !x->defined()) return nullptr;
    TORCH_CHECK(x->device() == dev && x->scalar_type() == st && x->is_contiguous() && x->numel() == numel, name,
                " must be a contiguous ", st, " tensor of ", numel, " elements on ", dev);
    return ptr(*x);
  };
  a.logw = f32(logw, m * k, "logw");
  a.score = f32(score, m * k, "score");
  a.u = f32(u, m, "u");
  a.weight = f32(weight, m * k, "weight");
  a.estimate = f32(estimate, 2 * m, "estimate");
  a.ess = f32(ess, m, "ess");
  a.index = reinterpret_cast<int32_t *>(typed(index, at::kInt, m * k, "index"));
  a.poses_out = f32(poses_out, 2 * m * k, "poses_out");
  a.logw_out = f32(logw_out, m * k, "logw_out");
  a.resampled = reinterpret_cast<uint8_t *>(typed(resampled, at::kByte, m, "resampled"));
  if (err.has_value() && err->defined()) {
    TORCH_CHECK(err->device() == dev && err->scalar_type() == at::kInt && err->numel() == 1,
                "err must be an int32 [1] tensor on ", dev);
    a.err = reinterpret_cast<uint32_t *>(err->data_ptr());
  }
  a.m = m;
  a.k = (int32_t)k;
  a.score_scale = (float)score_scale;
  a.ess_frac = (float)ess_frac;
  if (m == 0) return;
  check(apg_lidar_pf_resample(&a, stream_of(dev)), "apg_lidar_pf_resample");
}

// The scan spread of a particle belief per candidate action (apg_lidar_scan_spread).  bits: int64
// [n_src, H, ceil(width / 64)]; poses: float32 [M, A, K, 2]; weight: float32 [M, K] or None; map_ids: int64 [M] or
// None; beam_dirs: float32 [B, 2]; spread: float32 [M, A] or None; mean: float32 [M, A, B] or None; err: int32 [1] or
// None.
void lidar_scan_spread(const at::Tensor &bits, int64_t width, const at::Tensor &poses,
                       const c10::optional<at::Tensor> &weight, const c10::optional<at::Tensor> &map_ids,
                       const at::Tensor &beam_dirs, double lidar_range, const c10::optional<at::Tensor> &spread,
                       const c10::optional<at::Tensor> &mean, const c10::optional<at::Tensor> &err) {
  TORCH_CHECK(bits.is_cuda(), "bits must be on a GPU device, got ", bits.device());
  const at::Device dev = bits.device();
  const c10::DeviceGuard guard(dev);
  TORCH_CHECK(bits.scalar_type() == at::kLong && bits.dim() == 3 && bits.is_contiguous(),
              "bits must be a contiguous int64 [n_src, H, ceil(width / 64)] tensor");
  TORCH_CHECK(width >= 1 && width <= 511 && bits.size(2) == (width + 63) / 64, "bits has ", bits.size(2),
              " words per row, width ", width, " needs ", (width + 63) / 64, " (width 1..511)");
  TORCH_CHECK(poses.dim() == 4 && poses.size(3) == 2, "poses must be [M, A, K, 2]");
  const int64_t m = poses.size(0), na = poses.size(1), k = poses.size(2);
  TORCH_CHECK(na >= 1 && na <= INT32_MAX, "poses: A must be >= 1, got ", na);
  TORCH_CHECK(k >= 1 && k <= 4096, "poses: K must be in 1..4096, got ", k);
  check_io(poses, dev, 2 * m * na * k, "poses");
  TORCH_CHECK(beam_dirs.dim() == 2 && beam_dirs.size(1) == 2, "beam_dirs must be [B, 2]");
  const int64_t b = beam_dirs.size(0);
  TORCH_CHECK(b >= 1 && b <= 1024, "beam_dirs: B must be in 1..1024, got ", b);
  check_io(beam_dirs, dev, 2 * b, "beam_dirs");
  apg_scan_spread_args a{};
  a.occ = reinterpret_cast<const uint64_t *>(ptr(bits));
  a.poses = reinterpret_cast<const float *>(ptr(poses));
  a.beam_dirs = reinterpret_cast<const float *>(ptr(beam_dirs));
  if (weight.has_value() && weight->defined()) {
    check_io(*weight, dev, m * k, "weight");
    a.weight = reinterpret_cast<const float *>(ptr(*weight));
  }
  if (map_ids.has_value() && map_ids->defined()) {
    TORCH_CHECK(map_ids->device() == dev && map_ids->scalar_type() == at::kLong && map_ids->dim() == 1 &&
                    map_ids->is_contiguous() && map_ids->numel() == m,
                "map_ids must be a contiguous int64 [M] tensor on ", dev);
    a.map_ids = reinterpret_cast<const int64_t *>(ptr(*map_ids));
  }
  if (spread.has_value() && spread->defined()) {
    check_io(*spread, dev, m * na, "spread");
    a.spread = reinterpret_cast<float *>(ptr(*spread));
  }
  if (mean.has_value() && mean->defined()) {
    check_io(*mean, dev, m * na * b, "mean");
    a.mean = reinterpret_cast<float *>(ptr(*mean));
  }
  if (err.has_value() && err->defined()) {
    TORCH_CHECK(err->device() == dev && err->scalar_type() == at::kInt && err->numel() == 1,
                "err must be an int32 [1] tensor on ", dev);
    a.err = reinterpret_cast<uint32_t *>(err->data_ptr());
  }
  a.n_src = bits.size(0);
  a.m = m;
  a.height = (int32_t)bits.size(1);
  a.width = (int32_t)width;
  a.a = (int32_t)na;
  a.k = (int32_t)k;
  a.beams = (int32_t)b;
  a.lidar_range = (float)lidar_range;
  if (m == 0) return;
  check(apg_lidar_scan_spread(&a, stream_of(dev)), "apg_lidar_scan_spread");
}

// Glimpses and fused match scores of the image envs at caller-chosen positions (apg_image_glimpse_scores).  pool: the
// image pool as the envs hold it (uint8 with APG_U8_POOL_PAD readable bytes behind it, row-major or RGBX tiles, or
// float32); geo: height, width, pool_channels, channels, pool_dtype, sensor_h, sensor_w, pool_len; index: int64 [M];
// positions: float64 or float32 [M, K, 2]; observed: float32 [M, s0, s1, C] or None (needed with score); score:
// float32 [M, K] or None; glimpse: float32 [M, K, s0, s1, C] or None; err: int32 [1] or None.
void image_glimpse_scores(const at::Tensor &pool, std::vector<int64_t> geo, double sensor_scale, const at::Tensor &index,
                          const at::Tensor &positions, const c10::optional<at::Tensor> &observed,
                          const c10::optional<at::Tensor> &score, const c10::optional<at::Tensor> &glimpse,
                          const c10::optional<at::Tensor> &err) {
  TORCH_CHECK(pool.is_cuda(), "pool must be on a GPU device, got ", pool.device());
  const at::Device dev = pool.device();
  const c10::DeviceGuard guard(dev);
  TORCH_CHECK(geo.size() == 8, "geo: height, width, pool_channels, channels, pool_dtype, sensor_h, sensor_w, pool_len");
  for (int i = 0; i < 7; i++) TORCH_CHECK(geo[i] >= 0 && geo[i] <= INT32_MAX, "geo[", i, "] out of range");
  apg_image_config c{};
  c.num_envs = c.num_envs_total = 1;
  c.kind = APG_IMAGE_LOCALIZE;
  c.step_limit = 1;
  c.height = (int32_t)geo[0];
  c.width = (int32_t)geo[1];
  c.pool_channels = (int32_t)geo[2];
  c.channels = (int32_t)geo[3];
  c.pool_dtype = (int32_t)geo[4];
  c.sensor_h = (int32_t)geo[5];
  c.sensor_w = (int32_t)geo[6];
  c.pool_len = geo[7];
  c.sensor_scale = sensor_scale;
  TORCH_CHECK(pool.is_contiguous(), "pool must be contiguous");
  TORCH_CHECK(pool.scalar_type() == (c.pool_dtype == APG_POOL_F32 ? at::kFloat : at::kByte),
              "pool must be ", c.pool_dtype == APG_POOL_F32 ? "float32" : "uint8", " for this pool_dtype");
  const int64_t img = c.pool_dtype == APG_POOL_U8_TILED
                          ? ((geo[0] + 3) / 4) * ((geo[1] + 7) / 8) * 128
                          : geo[0] * geo[1] * geo[2];
  TORCH_CHECK(c.pool_len >= 1 && pool.numel() == c.pool_len * img, "pool must hold pool_len images of ", img,
              " elements, got ", pool.numel());
  if (c.pool_dtype != APG_POOL_F32)
    TORCH_CHECK((int64_t)pool.storage().nbytes() - pool.storage_offset() >= pool.numel() + APG_U8_POOL_PAD,
                "a uint8 pool needs APG_U8_POOL_PAD readable bytes behind it in its allocation");
  TORCH_CHECK(positions.dim() == 3 && positions.size(2) == 2, "positions must be [M, K, 2]");
  const int64_t m = positions.size(0), k = positions.size(1);
  TORCH_CHECK(k <= INT32_MAX, "positions: too many positions per set");
  TORCH_CHECK(positions.device() == dev && positions.is_contiguous() &&
                  (positions.scalar_type() == at::kDouble || positions.scalar_type() == at::kFloat),
              "positions must be a contiguous float64 or float32 tensor on ", dev);
  TORCH_CHECK(index.device() == dev && index.scalar_type() == at::kLong && index.dim() == 1 && index.is_contiguous() &&
                  index.numel() == m,
              "index must be a contiguous int64 [M] tensor on ", dev);
  const int64_t l = geo[5] * geo[6] * geo[3];
  const float *obs = nullptr;
  float *sc = nullptr, *gl = nullptr;
  uint32_t *errp = nullptr;
  if (observed.has_value() && observed->defined()) {
    check_io(*observed, dev, m * l, "observed");
    obs = reinterpret_cast<const float *>(ptr(*observed));
  }
  if (score.has_value() && score->defined()) {
    check_io(*score, dev, m * k, "score");
    TORCH_CHECK(obs || m * l == 0, "score needs observed");
    sc = reinterpret_cast<float *>(ptr(*score));
  }
  if (glimpse.has_value() && glimpse->defined()) {
    check_io(*glimpse, dev, m * k * l, "glimpse");
    gl = reinterpret_cast<float *>(ptr(*glimpse));
  }
  if (err.has_value() && err->defined()) {
    TORCH_CHECK(err->device() == dev && err->scalar_type() == at::kInt && err->numel() == 1,
                "err must be an int32 [1] tensor on ", dev);
    errp = reinterpret_cast<uint32_t *>(err->data_ptr());
  }
  if (m * k == 0 || (!sc && !gl)) return;
  check(apg_image_glimpse_scores(&c, ptr(pool), reinterpret_cast<const int64_t *>(ptr(index)), ptr(positions),
                                 positions.scalar_type() == at::kFloat ? 1 : 0, m, (int32_t)k, obs, sc, gl, errp,
                                 stream_of(dev)),
        "apg_image_glimpse_scores");
}

// Open-loop rollouts of candidate actions with the image envs' move (apg_image_move).  start: float64 [M, 2];
// actions: float32 [M, K, T, 2]; pos: float64 [M, K, T, 2]; glimpse_pos: float32 [M, K, T, 2]; base_reward: float32
// [M, K, T]; err: int32 [1] or None.
void image_move(const at::Tensor &start, const at::Tensor &actions, double msl0, double msl1, int64_t max_steps,
                at::Tensor pos, at::Tensor glimpse_pos, at::Tensor base_reward, const c10::optional<at::Tensor> &err) {
  TORCH_CHECK(start.is_cuda(), "start must be on a GPU device, got ", start.device());
  const at::Device dev = start.device();
  const c10::DeviceGuard guard(dev);
  TORCH_CHECK(actions.dim() == 4 && actions.size(3) == 2, "actions must be [M, K, T, 2]");
  const int64_t m = actions.size(0), k = actions.size(1), t = actions.size(2);
  TORCH_CHECK(k <= INT32_MAX && t >= 1 && t <= 4096, "actions: T must be in [1, 4096]");
  TORCH_CHECK(max_steps >= 0, "max_steps must be >= 0");
  TORCH_CHECK(start.scalar_type() == at::kDouble && start.is_contiguous() && start.numel() == 2 * m,
              "start must be a contiguous float64 [M, 2] tensor");
  check_io(actions, dev, 2 * m * k * t, "actions");
  TORCH_CHECK(pos.device() == dev && pos.scalar_type() == at::kDouble && pos.is_contiguous() &&
                  pos.numel() == 2 * m * k * t,
              "pos must be a contiguous float64 [M, K, T, 2] tensor on ", dev);
  check_io(glimpse_pos, dev, 2 * m * k * t, "glimpse_pos");
  check_io(base_reward, dev, m * k * t, "base_reward");
  uint32_t *errp = nullptr;
  if (err.has_value() && err->defined()) {
    TORCH_CHECK(err->device() == dev && err->scalar_type() == at::kInt && err->numel() == 1,
                "err must be an int32 [1] tensor on ", dev);
    errp = reinterpret_cast<uint32_t *>(err->data_ptr());
  }
  if (m * k == 0) return;
  apg_image_config c{};
  c.max_step[0] = msl0;
  c.max_step[1] = msl1;
  check(apg_image_move(&c, reinterpret_cast<const double *>(ptr(start)), reinterpret_cast<const float *>(ptr(actions)),
                       m, (int32_t)k, (int32_t)t, (int32_t)std::min<int64_t>(max_steps, INT32_MAX),
                       reinterpret_cast<double *>(ptr(pos)), reinterpret_cast<float *>(ptr(glimpse_pos)),
                       reinterpret_cast<float *>(ptr(base_reward)), errp, stream_of(dev)),
        "apg_image_move");
}

// Overlap scores of target-position hypotheses from a localization env's own observations
// (apg_image_overlap_scores).  glimpse, target_glimpse: float32 [M, s0, s1, C]; glimpse_pos: float64 or float32
// [M, 2]; hypotheses: float64 or float32 [M, K, 2] or [K, 2] (shared by every set); image_size: H, W; logw, logw_out:
// float32 [M, K], both or neither (logw_out may be logw itself); sse: float32 [M, K]; count: int32 [M, K]; err: int32
// [1] or None.
void image_overlap_scores(const at::Tensor &glimpse, const at::Tensor &glimpse_pos, const at::Tensor &target_glimpse,
                          const at::Tensor &hypotheses, std::vector<int64_t> image_size, double sensor_scale,
                          const c10::optional<at::Tensor> &logw, double gain, double tau, at::Tensor sse,
                          at::Tensor count, const c10::optional<at::Tensor> &logw_out,
                          const c10::optional<at::Tensor> &err) {
  TORCH_CHECK(glimpse.is_cuda(), "glimpse must be on a GPU device, got ", glimpse.device());
  const at::Device dev = glimpse.device();
  const c10::DeviceGuard guard(dev);
  TORCH_CHECK(glimpse.dim() == 4, "glimpse must be [M, s0, s1, C]");
  TORCH_CHECK(image_size.size() == 2 && image_size[0] >= 2 && image_size[0] <= INT32_MAX && image_size[1] >= 2 &&
                  image_size[1] <= INT32_MAX,
              "image_size: (H, W), each >= 2");
  const int64_t m = glimpse.size(0), s0 = glimpse.size(1), s1 = glimpse.size(2), ch = glimpse.size(3);
  TORCH_CHECK(s0 >= 1 && s1 >= 1 && ch >= 1 && s0 <= 4096 && s1 <= 4096 && ch <= 4096 && s0 * s1 * ch <= 4096,
              "a glimpse holds 1..4096 values, got ", s0, " x ", s1, " x ", ch);
  const int64_t l = s0 * s1 * ch;
  check_io(glimpse, dev, m * l, "glimpse");
  check_io(target_glimpse, dev, m * l, "target_glimpse");
  auto is_pos = [&](const at::Tensor &t) {
    return t.device() == dev && t.is_contiguous() && (t.scalar_type() == at::kDouble || t.scalar_type() == at::kFloat);
  };
  TORCH_CHECK(is_pos(glimpse_pos) && glimpse_pos.numel() == 2 * m,
              "glimpse_pos must be a contiguous float64 or float32 [M, 2] tensor on ", dev);
  const bool shared = hypotheses.dim() == 2;
  TORCH_CHECK((hypotheses.dim() == 3 && hypotheses.size(0) == m && hypotheses.size(2) == 2) ||
                  (shared && hypotheses.size(1) == 2),
              "hypotheses must be [M, K, 2] or [K, 2]");
  TORCH_CHECK(is_pos(hypotheses), "hypotheses must be a contiguous float64 or float32 tensor on ", dev);
  const int64_t k = hypotheses.size(shared ? 0 : 1);
  TORCH_CHECK(k <= INT32_MAX, "hypotheses: too many per set");
  apg_overlap_scores_args a{};
  auto f32 = [&](const c10::optional<at::Tensor> &x, const char *name) -> float * {
    if (!x.has_value() || !x->defined()) return nullptr;
    check_io(*x, dev, m * k, name);
    return reinterpret_cast<float *>(x->data_ptr());
  };
  a.logw = f32(logw, "logw");
  a.logw_out = f32(logw_out, "logw_out");
  TORCH_CHECK((logw.has_value() && logw->defined()) == (logw_out.has_value() && logw_out->defined()),
              "logw and logw_out go together");
  check_io(sse, dev, m * k, "sse");
  TORCH_CHECK(count.device() == dev && count.scalar_type() == at::kInt && count.is_contiguous() &&
                  count.numel() == m * k,
              "count must be a contiguous int32 tensor of ", m * k, " elements on ", dev);
  if (err.has_value() && err->defined()) {
    TORCH_CHECK(err->device() == dev && err->scalar_type() == at::kInt && err->numel() == 1,
                "err must be an int32 [1] tensor on ", dev);
    a.err = reinterpret_cast<uint32_t *>(err->data_ptr());
  }
  if (m * k == 0) return;
  a.glimpse = reinterpret_cast<const float *>(ptr(glimpse));
  a.target_glimpse = reinterpret_cast<const float *>(ptr(target_glimpse));
  a.glimpse_pos = ptr(glimpse_pos);
  a.hypotheses = ptr(hypotheses);
  a.sse = reinterpret_cast<float *>(ptr(sse));
  a.count = reinterpret_cast<int32_t *>(ptr(count));
  a.m = m;
  a.k = (int32_t)k;
  a.height = (int32_t)image_size[0];
  a.width = (int32_t)image_size[1];
  a.sensor_h = (int32_t)s0;
  a.sensor_w = (int32_t)s1;
  a.channels = (int32_t)ch;
  a.pos_is_f32 = glimpse_pos.scalar_type() == at::kFloat;
  a.hyp_is_f32 = hypotheses.scalar_type() == at::kFloat;
  a.hyp_shared = shared;
  a.gain = (float)gain;
  a.tau = (float)tau;
  a.sensor_scale = sensor_scale;
  check(apg_image_overlap_scores(&a, stream_of(dev)), "apg_image_overlap_scores");
}

}  // namespace

TORCH_LIBRARY(apgym, m) {
  m.class_<LidarEnv>("LidarEnv")
      .def(torch::init<std::vector<int64_t>, std::vector<double>, std::vector<at::Tensor>, std::vector<at::Tensor>>());
  m.class_<ImageEnv>("ImageEnv")
      .def(torch::init<std::vector<int64_t>, std::vector<double>, std::vector<at::Tensor>, std::vector<at::Tensor>>());
  m.def("lidar_reset(__torch__.torch.classes.apgym.LidarEnv env, int seed, bool use_seed) -> ()", lidar_reset);
  m.def("lidar_step(__torch__.torch.classes.apgym.LidarEnv env, Tensor action, Tensor prediction) -> ()", lidar_step);
  m.def("image_reset(__torch__.torch.classes.apgym.ImageEnv env) -> ()", image_reset);
  m.def("image_step(__torch__.torch.classes.apgym.ImageEnv env, Tensor action, Tensor prediction, int t, "
        "int prev_done) -> ()",
        image_step);
  m.def("unpack_map_bits(Tensor bits, int width, Tensor? env_ids, Tensor(a!) out, float wall, Tensor(b!)? err=None) "
        "-> ()",
        unpack_map_bits);
  m.def("lidar_scan_poses(Tensor bits, int width, Tensor poses, Tensor? map_ids, Tensor beam_dirs, float lidar_range, "
        "bool normalize, Tensor? observed, Tensor(a!)? scan, Tensor(b!)? score, Tensor(c!)? err) -> ()",
        lidar_scan_poses);
  m.def("lidar_move_poses(Tensor bits, int width, Tensor poses, Tensor actions, Tensor? map_ids, Tensor? max_steps, "
        "Tensor? origin, Tensor? origin_alias, Tensor(a!) pos, Tensor(b!) steps, Tensor(c!) terminated, "
        "Tensor(d!)? base_reward, Tensor(e!)? odometry, Tensor(f!)? err) -> ()",
        lidar_move_poses);
  m.def("lidar_pf_resample(Tensor poses, Tensor? logw, Tensor? score, Tensor? u, float score_scale, "
        "float ess_frac, Tensor(a!)? weight, Tensor(b!)? estimate, Tensor(c!)? ess, Tensor(d!)? index, "
        "Tensor(e!)? poses_out, Tensor(f!)? logw_out, Tensor(g!)? resampled, Tensor(h!)? err) -> ()",
        lidar_pf_resample);
  m.def("lidar_scan_spread(Tensor bits, int width, Tensor poses, Tensor? weight, Tensor? map_ids, Tensor beam_dirs, "
        "float lidar_range, Tensor(a!)? spread, Tensor(b!)? mean, Tensor(c!)? err) -> ()",
        lidar_scan_spread);
  m.def("image_glimpse_scores(Tensor pool, int[] geo, float sensor_scale, Tensor index, Tensor positions, "
        "Tensor? observed, Tensor(a!)? score, Tensor(b!)? glimpse, Tensor(c!)? err) -> ()",
        image_glimpse_scores);
  m.def("image_move(Tensor start, Tensor actions, float msl0, float msl1, int max_steps, Tensor(a!) pos, "
        "Tensor(b!) glimpse_pos, Tensor(c!) base_reward, Tensor(d!)? err) -> ()",
        image_move);
  m.def("image_overlap_scores(Tensor glimpse, Tensor glimpse_pos, Tensor target_glimpse, Tensor hypotheses, "
        "int[] image_size, float sensor_scale, Tensor? logw, float gain, float tau, Tensor(a!) sse, Tensor(b!) count, "
        "Tensor(c!)? logw_out, Tensor(d!)? err) -> ()",
        image_overlap_scores);
}
