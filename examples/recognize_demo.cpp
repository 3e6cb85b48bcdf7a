/*
 * recognize_demo.cpp — labels without a detector: every model file is trained (PPF3DDetector::trainModel), prep::Recognizer
 * builds the models' pair-feature key sets once (ppf_recognizer_create), and the proposal cloud is scored against all of them
 * (ppf_recognize_frame).  Prints each model's key set, the proposal's used rows and its candidates, best first -- the first is
 * the model Cloud::matchFrame should be given for this proposal.
 *
 *   usage: recognize_demo proposal.f32 rows model.f32 rows [model.f32 rows ...] [--top k] [--max-rows n] [--min-score s]
 *          (raw little-endian files: rows x 6 float32, x y z nx ny nz)
 *   build: g++ -std=c++11 -Iinclude examples/recognize_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
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

static vector<float> read_rows(const char* path, int rows) {
  if (rows <= 0) throw ppf_match_3d::Error(PPF_ERR_INVALID, string("rows of ") + path + " must be positive");
  vector<float> a((size_t)rows * 6);
  ifstream f(path, ios::binary);
  if (!f.read(reinterpret_cast<char*>(&a[0]), (streamsize)(a.size() * sizeof(float))))
    throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + path);
  return a;
}

int main(int argc, char** argv) {
  vector<const char*> files;
  ppf_recognize_params rp = prep::Recognizer::defaultParams();
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--top") && i + 1 < argc) rp.top = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--max-rows") && i + 1 < argc) rp.max_rows = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--min-score") && i + 1 < argc) rp.min_score = atof(argv[++i]);
    else files.push_back(argv[i]);
  }
  if (files.size() < 4 || files.size() % 2 != 0) {
    cerr << "usage: " << argv[0] << " proposal.f32 rows model.f32 rows [model.f32 rows ...] [--top k] [--max-rows n] [--min-score s]" << endl;
    return 1;
  }
  try {
    const vector<float> view = read_rows(files[0], atoi(files[1]));
    vector<ppf_match_3d::PPF3DDetector> detectors((files.size() - 2) / 2, ppf_match_3d::PPF3DDetector(0.05, 0.05));
    vector<const ppf_model*> models;
    for (size_t m = 0; m < detectors.size(); m++) {
      const int rows = atoi(files[3 + 2 * m]);
      const vector<float> cloud = read_rows(files[2 + 2 * m], rows);
      detectors[m].trainModel(&cloud[0], rows, 6);
      models.push_back(detectors[m].handle());
    }
    const prep::Recognizer rec(models);
    for (int m = 0; m < rec.models(); m++) {
      const ppf_recognizer_info mi = rec.modelInfo(m);
      printf("model %d %s rows %d keys %llu bins %d %d %d %d bytes %llu %s\n", m, files[2 + 2 * (size_t)m], mi.n_rows, (unsigned long long)mi.n_keys,
             mi.n_bins[0], mi.n_bins[1], mi.n_bins[2], mi.n_bins[3], (unsigned long long)mi.bytes, mi.in_lds ? "lds" : "global");
    }
    const prep::Cloud proposal = prep::Cloud::fromRows(&view[0], (int)(view.size() / 6), 6, 6);
    vector<const prep::Cloud*> clouds(1, &proposal);
    vector<int32_t> used;
    ppf_recognize_stats st;
    const vector<vector<ppf_recognize_score> > ranked = rec.recognize(clouds, &rp, &used, 0, &st);
    printf("used rows %d launches %d waits %d\n", used[0], st.n_launches, st.n_host_syncs);
    for (size_t k = 0; k < ranked[0].size(); k++)
      printf("candidate %d model %d score %.6f precision %.6f recall %.6f known %llu keys_hit %llu\n", (int)k, ranked[0][k].model, ranked[0][k].score,
             ranked[0][k].precision, ranked[0][k].recall, (unsigned long long)ranked[0][k].n_known, (unsigned long long)ranked[0][k].n_keys_hit);
    if (ranked[0].empty()) printf("no candidate: clutter\n");
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
