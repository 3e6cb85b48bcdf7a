/*
 * frame_refine_demo.cpp — the post-detector half of the reference's driver for every detection of a frame, with the poses
 * fitted to the depth image itself at the end: Cloud::prepareFrame, Cloud::matchFrame (Matching_S2B + ICP of the top 8 poses
 * of every detection), Cloud::selectFrame (one consistent set), then Cloud::refineFrame on the selected poses (polish).
 * With a second depth image of the same camera the refined poses are then refined against it as well (tracking: last
 * frame's poses against this frame's depth, no matching).  Every box is matched against the one model given.  Prints one
 * line per selected pose and refinement with its info row and the refined matrix.
 *
 *   usage: frame_refine_demo scene_xyz.f32 n_points depth.f32 rows cols fx fy ppx ppy boxes.i32 n_boxes model_xyzn.f32 n_model
 *          [min_score [next_depth.f32]]
 *          (raw little-endian files: scene n x 3 float32, depth rows x cols float32 metres, boxes n x 4 int32 {x y w h},
 *           model n x 6 float32 x y z nx ny nz)
 *   build: g++ -std=c++11 -Iinclude examples/frame_refine_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ppf_cloud_stages.hpp"

using namespace std;
using namespace ppfhip;

template <class T>
static void read_raw(const char* path, vector<T>& v, size_t count) {
  ifstream f(path, ios::binary);
  if (!f.read(reinterpret_cast<char*>(&v[0]), (streamsize)(count * sizeof(T))))
    throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + path);
}

static void report(const char* what, const vector<pair<int, int> >& chosen, const vector<vector<ppf_match_3d::Pose3D> >& poses,
                   const vector<vector<ppf_refine_info> >& info) {
  for (size_t r = 0; r < chosen.size(); r++) {
    const ppf_refine_info& f = info[r][0];
    const ppf_pose p = poses[r][0].record();
    printf("%s det %d k %d: status %d iterations %d n_rows %d n_considered %d n_pairs_first %d n_pairs_last %d rmse_first %.9g rmse_last %.9g pose",
           what, chosen[r].first, chosen[r].second, f.status, f.iterations, f.n_rows, f.n_considered, f.n_pairs_first, f.n_pairs_last,
           (double)f.rmse_first, (double)f.rmse_last);
    for (int e = 0; e < 16; e++) printf(" %.17g", p.pose[e]);
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 14) {
    cerr << "usage: " << argv[0]
         << " scene_xyz.f32 n_points depth.f32 rows cols fx fy ppx ppy boxes.i32 n_boxes model_xyzn.f32 n_model [min_score [next_depth.f32]]"
         << endl;
    return 1;
  }
  try {
    const int n = atoi(argv[2]), rows = atoi(argv[4]), cols = atoi(argv[5]), nb = atoi(argv[11]), nm = atoi(argv[13]);
    vector<float> xyz((size_t)n * 3 + 1), depth((size_t)rows * cols), model((size_t)nm * 6 + 1);
    vector<int> boxes((size_t)nb * 4 + 1);
    read_raw(argv[1], xyz, (size_t)n * 3);
    read_raw(argv[3], depth, depth.size());
    if (nb) read_raw(argv[10], boxes, (size_t)nb * 4);
    read_raw(argv[12], model, (size_t)nm * 6);
    const double fx = atof(argv[6]), fy = atof(argv[7]), ppx = atof(argv[8]), ppy = atof(argv[9]);

    prep::Cloud scene = prep::Cloud::fromXYZ(&xyz[0], n);
    const vector<pair<prep::Cloud, prep::Cloud> > dets = scene.prepareFrame(&boxes[0], nb, &depth[0], rows, cols, fx, fy, ppx, ppy);
    ppf_match_3d::PPF3DDetector detector(0.05, 0.05);
    detector.trainModel(&model[0], nm, 6);
    const prep::Cloud modelCloud = prep::Cloud::fromRows(&model[0], nm, 6, 6);
    const vector<const ppf_model*> models(dets.size(), detector.handle());
    const vector<const prep::Cloud*> modelClouds(dets.size(), &modelCloud);
    const vector<vector<ppf_match_3d::Pose3D> > poses = prep::Cloud::matchFrame(models, modelClouds, dets, 0.05, 0.05, 8);
    ppf_select_params sp;
    ppf_default_select_params(&sp);
    if (argc > 14) sp.min_score = (float)atof(argv[14]);
    const vector<pair<int, int> > chosen = prep::Cloud::selectFrame(modelClouds, poses, &depth[0], rows, cols, fx, fy, ppx, ppy, &sp);

    /* one "detection" per selected pose */
    vector<vector<ppf_match_3d::Pose3D> > held;
    for (size_t r = 0; r < chosen.size(); r++)
      held.push_back(vector<ppf_match_3d::Pose3D>(1, poses[(size_t)chosen[r].first][(size_t)chosen[r].second]));
    const vector<const prep::Cloud*> heldClouds(held.size(), &modelCloud);
    vector<vector<ppf_refine_info> > info;
    ppf_refine_stats st;
    held = prep::Cloud::refineFrame(heldClouds, held, &depth[0], rows, cols, fx, fy, ppx, ppy, 0, &info, &st);
    report("polish", chosen, held, info);
    printf("jobs %d launches %d read-backs %d\n", st.n_jobs, st.n_launches, st.n_host_syncs);
    if (argc > 15) {
      vector<float> next((size_t)rows * cols);
      read_raw(argv[15], next, next.size());
      held = prep::Cloud::refineFrame(heldClouds, held, &next[0], rows, cols, fx, fy, ppx, ppy, 0, &info, &st);
      report("track", chosen, held, info);
    }
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
