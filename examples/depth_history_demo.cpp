/*
 * depth_history_demo.cpp — a stream from a fixed camera fused before anything is built on it: prep::DepthHistory
 * (ppf_depth_history: the last `window` frames on the device, each push one fused image) -> prep::filterDepth ->
 * Cloud::fromDepth with ppf_depth_normal_params.  The stream is the given depth image pushed `frames` times, each time with
 * seeded noise and about one pixel in ten dropped, so the fused image has less noise than any frame and no hole a frame has.
 * Prints every push's counts, then checksums of the bytes (the sum of the 32-bit words, of the bytes for the state image).
 *
 * The noise of pixel i of frame f is a hash of seed + f * rows * cols + i (64-bit, wrapping):
 *   h = x * 0x9E3779B97F4A7C15; h ^= h >> 32; h *= 0xD6E8FEB86659FD93; h ^= h >> 32
 *   dropped iff ((h >> 16) & 255) < 26;  else z' = (float)((double)z + noise * ((double)(h & 65535) / 65536.0 - 0.5))
 *
 *   usage: depth_history_demo depth.f32 rows cols fx fy ppx ppy [frames [window [range_abs [range_quad [min_support [max_age
 *          [flags [noise [seed]]]]]]]]]
 *          (raw little-endian file: rows x cols float32 metres)
 *   build: g++ -std=c++11 -Iinclude examples/depth_history_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ppf_cloud_stages.hpp"

using namespace std;
using namespace ppfhip;

static unsigned long long checksum(const vector<float>& a, unsigned long long sum = 0) {
  uint32_t w;
  for (size_t i = 0; i < a.size(); i++) { memcpy(&w, &a[i], sizeof(w)); sum += w; }
  return sum;
}

static void noisy(const vector<float>& depth, int frame, double noise, uint64_t seed, vector<float>& out) {
  const uint64_t n = depth.size();
  out.resize(depth.size());
  for (uint64_t i = 0; i < n; i++) {
    uint64_t h = (seed + (uint64_t)frame * n + i) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    const bool dropped = ((h >> 16) & 255u) < 26u;
    out[i] = dropped ? 0.f : (float)((double)depth[i] + noise * ((double)(h & 65535u) / 65536.0 - 0.5));
  }
}

int main(int argc, char** argv) {
  if (argc < 8) {
    cerr << "usage: " << argv[0]
         << " depth.f32 rows cols fx fy ppx ppy [frames [window [range_abs [range_quad [min_support [max_age [flags [noise "
            "[seed]]]]]]]]]" << endl;
    return 1;
  }
  try {
    const int rows = atoi(argv[2]) > 0 ? atoi(argv[2]) : 0, cols = atoi(argv[3]) > 0 ? atoi(argv[3]) : 0;
    if (rows == 0 || cols == 0) throw ppf_match_3d::Error(PPF_ERR_INVALID, "rows and cols must be positive");
    vector<float> depth((size_t)rows * (size_t)cols + 1);
    ifstream f(argv[1], ios::binary);
    if (!f.read(reinterpret_cast<char*>(&depth[0]), (streamsize)((size_t)rows * (size_t)cols * sizeof(float))))
      throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + argv[1]);
    depth.resize((size_t)rows * (size_t)cols);
    const double intr[4] = {atof(argv[4]), atof(argv[5]), atof(argv[6]), atof(argv[7])};
    const int frames = argc > 8 ? atoi(argv[8]) : 8;
    ppf_depth_history_params hp = prep::DepthHistory::defaultParams();
    if (argc > 9) hp.window = atoi(argv[9]);
    if (argc > 10) hp.range_abs = (float)atof(argv[10]);
    if (argc > 11) hp.range_quad = (float)atof(argv[11]);
    if (argc > 12) hp.min_support = atoi(argv[12]);
    if (argc > 13) hp.max_age = atoi(argv[13]);
    if (argc > 14) hp.flags = atoi(argv[14]);
    const double noise = argc > 15 ? atof(argv[15]) : 0.004;
    const uint64_t seed = argc > 16 ? (uint64_t)strtoull(argv[16], 0, 10) : 1u;

    prep::DepthHistory history(rows, cols, &hp);
    vector<float> frame, fused;
    vector<uint8_t> state;
    for (int k = 0; k < frames; k++) {
      noisy(depth, k, noise, seed, frame);
      ppf_depth_history_stats st;
      fused = history.push(&frame[0], &state, &st);
      printf("frame %lld kept %d measured %d filled %d unsupported %d empty %d changed %d\n", (long long)st.frame, st.n_kept,
             st.n_measured, st.n_filled, st.n_unsupported, st.n_empty, st.n_changed);
    }
    unsigned long long ssum = 0;
    for (size_t i = 0; i < state.size(); i++) ssum += state[i];
    const ppf_depth_history_desc d = history.info();
    printf("history %d x %d window %d frames %lld\n", d.rows, d.cols, d.window, (long long)d.frames);
    printf("fused image checksum %llu state checksum %llu\n", checksum(fused), ssum);
    if (frames > 0) {
      ppf_depth_filter_stats fs;
      const vector<float> filtered = prep::filterDepth(&fused[0], rows, cols, 0, 0.f, 0.f, 0, &fs);
      printf("filtered kept %d unsupported %d written %d checksum %llu\n", fs.n_kept, fs.n_unsupported, fs.n_written, checksum(filtered));
      const prep::Cloud scene = prep::Cloud::fromDepth(&filtered[0], rows, cols, prep::Cloud::defaultDepthNormalParams(), intr[0], intr[1],
                                                       intr[2], intr[3], 0.f, 0.f, true);
      vector<float> r, curv;
      scene.download(r, curv);
      printf("cloud rows %d checksum %llu\n", scene.size(), checksum(curv, checksum(r)));
    }
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
