/*
 * ppf_model_host.h — C-ABI, model side: defaults, ppf_model_train (table build), handles, table dump, the versioned model file.
 * Reference call sites: /root/reference/include/CloudProcessing.h:205-261 (ctor, trainModel, write), :106-121 (read).
 *
 * What a model is made of is stated once each:
 *   model_plan    parameters + sampled row count + diameter -> steps, key dimensions, slots, tiles (pure; the refusals of training)
 *   build_table   the device passes of training over one TrainScratch: buckets, counts, dealing positions, fill
 *   ModelImage    the part of a model a file holds, on the host: image_sections sizes it, model_image_read / _write are the
 *                 file (read validates everything, without a device), model_download / model_upload are the only copies
 *   row_groups    the group records of the buckets that vote through count tables (pure; ppf_debug_model_row_groups)
 *   model_finish  what is derived once the table stands, after training and after loading alike: bucket_total, bucket_mid,
 *                 the key LUT, the group records, device_bytes
 */
#ifndef PPF_MODEL_HOST_H
#define PPF_MODEL_HOST_H

/* ============================================================================================ */
/* C-ABI                                                                                          */
/* ============================================================================================ */
extern "C" {

void ppf_default_train_params(ppf_train_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->relative_sampling_step = 0.05;
  p->relative_distance_step = 0.05;
  p->num_angles = 30;
}
void ppf_default_match_params(ppf_match_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->relative_scene_sample_step = 1.0 / 5.0;
  p->relative_scene_distance = 0.03;
  p->position_threshold = -1;
  p->rotation_threshold = -1;
  p->ref_stride = 1;
}
int ppf_abi_version(void) { return PPF_ABI_VERSION; }
int ppf_last_error(char* buf, int cap) {
  if (buf && cap > 0) {
    strncpy(buf, g_last_error.c_str(), (size_t)cap - 1);
    buf[cap - 1] = 0;
  }
  return (int)g_last_error.size();
}
int ppf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"

namespace {

/* ---- parameters -> plan ------------------------------------------------------------------------- */
/* model reference points whose accumulator rows fit one k_vote workgroup's LDS next to its fixed part */
int max_tile_rows(int num_angles) {
  const long budget = (long)LDS_BYTES - (long)VOTE_LDS_FIXED - 4L * (vote_guard(num_angles) + 1);
  return budget <= 0 ? 0 : (int)(budget / (4L * vote_pitch(num_angles)));
}
/* row codes below this one name the guard words: the padding entries of the pair records */
uint32_t first_real_row(int num_angles) { return (uint32_t)((vote_guard(num_angles) - num_angles) * 4); }

/* tabulate hash -> bucket for every key with angle bins 0..floor(pi/angle_step)+1 and distance bins 0..1023 (pairs up
 * to ~1000 distance steps apart: tens of model diameters); everything else keeps the hash path in k_pairs.
 * PPF_FEATURE_DARBOUX: the angle key spans -pi..pi and the two cosine keys -1..1, all divided by the angle step and floored. */
KeyDims key_lut_dims(int feature, double angle_step) {
  KeyDims d;
  if (feature == PPF_FEATURE_DARBOUX) {
    d.o0 = (int)std::floor(PPF_PI / angle_step) + 2;
    d.o1 = d.o2 = (int)std::floor(1.0 / angle_step) + 2;
    d.n0 = 2 * d.o0 + 1;
    d.n1 = d.n2 = 2 * d.o1 + 1;
  } else {
    d.o0 = d.o1 = d.o2 = 0;
    d.n0 = d.n1 = d.n2 = (int)std::floor(PPF_PI / angle_step) + 2;
  }
  d.nd = 1024;
  const size_t per_dist = (size_t)d.n0 * d.n1 * d.n2;
  if (per_dist * d.nd > ((size_t)1 << 26)) /* very fine angle steps: shrink the distance range to keep the table at 256 MiB */
    d.nd = (int)std::max<size_t>(1, ((size_t)1 << 26) / per_dist);
  return d;
}
/* hash slots of the table: next_pow2(N^2) like the reference's library, or (PPF_KEY_EXACT) one slot per quantised key */
uint32_t table_slots(int key_equality, const KeyDims& kd, int n_ref) {
  if (key_equality == PPF_KEY_EXACT) return next_pow2(std::max<uint32_t>((uint32_t)key_table_size(kd), 16u));
  return next_pow2(std::max<uint32_t>((uint32_t)((size_t)n_ref * n_ref), 16u));
}

/* What the parameters imply for a cloud of n_sampled rows and that diameter (the ctor + setSearchParams defaults of the
 * reference's detector): everything of ppf_model_info that is known before the table is built, the key dimensions, and
 * every refusal of training that needs no device. */
struct ModelPlan {
  ppf_model_info info; /* n_buckets, n_entries and device_bytes stay 0: build_table's */
  KeyDims kd;
  int max_refs;        /* rows a tile may hold */
};
ppf_status model_plan(int n_sampled, float diameter, const ppf_train_params& params, ModelPlan& plan) {
  plan = ModelPlan{};
  ppf_model_info& I = plan.info;
  const int N = n_sampled;
  if (N < 2 || (uint64_t)N * N > 0x7FFFFFFFull) return fail(PPF_ERR_INVALID, "ppf_model_train: %d sampled model points unsupported", N);
  const double angle_step = (360.0 / params.num_angles) * PPF_PI / 180.0;
  const float dist_step = (float)(diameter * (params.distance_from_distance_step ? params.relative_distance_step
                                                                                 : params.relative_sampling_step));
  I.n_ref = N;
  I.num_angles = (int)std::floor(2 * PPF_PI / angle_step);
  I.angle_step = angle_step;
  I.distance_step = dist_step;
  I.diameter = diameter;
  plan.kd = key_lut_dims(params.feature, angle_step);
  if (key_table_size(plan.kd) > ((size_t)1 << 30)) /* k_pairs indexes the key table with 32-bit arithmetic (and 4 GiB of keys would be pointless) */
    return fail(PPF_ERR_INVALID, "ppf_model_train: num_angles %g is too fine for the key table", params.num_angles);
  if (params.key_equality != PPF_KEY_BUCKET && params.key_equality != PPF_KEY_EXACT)
    return fail(PPF_ERR_INVALID, "ppf_model_train: key_equality must be PPF_KEY_BUCKET or PPF_KEY_EXACT");
  if (params.feature != PPF_FEATURE_PPF && params.feature != PPF_FEATURE_DARBOUX)
    return fail(PPF_ERR_INVALID, "ppf_model_train: feature must be PPF_FEATURE_PPF or PPF_FEATURE_DARBOUX");
  if (params.key_equality == PPF_KEY_EXACT && (double)diameter / (double)dist_step + 2.0 > (double)plan.kd.nd)
    return fail(PPF_ERR_INVALID, "ppf_model_train: PPF_KEY_EXACT needs diameter / distance step (%g) below %d", (double)diameter / dist_step, plan.kd.nd);
  I.slots = table_slots(params.key_equality, plan.kd, N);
  I.position_threshold_default = params.relative_sampling_step;
  I.rotation_threshold_default = ((360 / angle_step) / 180.0 * PPF_PI);
  plan.max_refs = 2 * max_tile_rows(I.num_angles); /* 16-bit cells: two rows per accumulator word */
  if (params.max_tile_refs > 0) plan.max_refs = std::min(plan.max_refs, params.max_tile_refs);
  if (plan.max_refs < 1) return fail(PPF_ERR_INVALID, "ppf_model_train: num_angles %d too large for the LDS accumulator", I.num_angles);
  I.n_tiles = (N + plan.max_refs - 1) / plan.max_refs;
  I.tile_refs = (N + I.n_tiles - 1) / I.n_tiles;
  return PPF_OK;
}

/* ---- the host image of a model -------------------------------------------------------------------- */
/* What a model file holds, and what training and loading put on the device before model_finish.  The element counts of
 * its arrays follow from the header alone (image_sections). */
struct ModelImage {
  ppf_train_params params{};
  ppf_model_info info{};
  uint64_t n_records = 0;
  std::vector<float> sampled;      /* n_ref x 6 */
  std::vector<SlotWord> slotmap;   /* slots / 64 */
  std::vector<uint32_t> bucket_off, bucket_slot; /* n_tiles x (n_buckets + 1) record offsets; n_buckets */
  std::vector<uint4> records;      /* n_records pair records */
};
enum : unsigned { IMG_SAMPLED = 1, IMG_SLOTMAP = 2, IMG_BUCKET_OFF = 4, IMG_BUCKET_SLOT = 8, IMG_RECORDS = 16, IMG_ALL = 31 };
struct ImageSections {
  uint64_t sampled, slotmap, bucket_off, bucket_slot, records; /* elements */
  uint64_t bytes() const {
    return sampled * sizeof(float) + slotmap * sizeof(SlotWord) + (bucket_off + bucket_slot) * sizeof(uint32_t) + records * sizeof(uint4);
  }
};
ImageSections image_sections(const ppf_model_info& I, uint64_t n_records) {
  const uint64_t nb = I.n_buckets;
  return {(uint64_t)I.n_ref * 6, ((uint64_t)I.slots + 63) / 64, (uint64_t)I.n_tiles * (nb + 1), nb, n_records};
}

/* ---- model (de)serialisation: versioned binary CSR (the reference's XML format is defined by a
 * private OpenCV patch and unknown) ------------------------------------------------- */
const char PPF_MAGIC[8] = {'P', 'P', 'F', 'H', 'I', 'P', '0', '5'}; /* 02: pair-record table; 03: ppf_train_params.feature; 04: 64 count-table cells (7-bit cell field), cell-grouped dealing; 05: the build's count-table cell count in the header */
/* what the records' count-table bits were computed with: a file written by a build with another PPF_AGG_Q carries cells of
 * another width in its row codes and would be voted through the wrong cells; it is refused */
struct ModelBuildWord { uint32_t agg_q, reserved; };
constexpr uint64_t IMAGE_HEADER_BYTES = 8 + sizeof(ModelBuildWord) + sizeof(ppf_train_params) + sizeof(ppf_model_info) + sizeof(uint64_t);

struct Closer { FILE* f; ~Closer() { if (f) fclose(f); } };

/* Everything read from the file is checked before it reaches a kernel: header fields against each other and against
 * the file size, the CSR rows, the record rows (LDS byte offsets k_vote adds to) and alphas, the slot map's ranks.
 * The two functions name the first check a header or a body fails, or return NULL. */
const char* image_header_fault(const ModelImage& im) {
  const ppf_model_info& I = im.info;
  const uint64_t N = (uint64_t)(I.n_ref > 0 ? I.n_ref : 0);
  if (I.n_ref < 2 || N * N > 0x7FFFFFFFull) return "n_ref";
  if (!(I.num_angles >= 1 && I.num_angles <= 4096) || !(I.angle_step > 1e-4) || !(I.distance_step > 0) || !std::isfinite(I.diameter)) return "steps";
  if (im.params.key_equality != PPF_KEY_BUCKET && im.params.key_equality != PPF_KEY_EXACT) return "key_equality";
  if (im.params.feature != PPF_FEATURE_PPF && im.params.feature != PPF_FEATURE_DARBOUX) return "feature";
  const KeyDims kd = key_lut_dims(im.params.feature, I.angle_step);
  if (key_table_size(kd) > ((size_t)1 << 30)) return "angle step too fine for the key table";
  if (I.slots != table_slots(im.params.key_equality, kd, I.n_ref)) return "slots";
  if (I.num_angles != (int)std::floor(2 * PPF_PI / I.angle_step)) return "num_angles";
  if (I.n_tiles < 1 || I.tile_refs < 1 || (uint64_t)I.n_tiles * I.tile_refs < N || (uint64_t)(I.n_tiles - 1) * I.tile_refs >= N)
    return "tiles";
  if (I.tile_refs > 2 * max_tile_rows(I.num_angles)) return "tile does not fit this build's LDS accumulator";
  if (I.n_buckets > I.slots || (uint64_t)I.n_buckets > N * N) return "n_buckets";
  if (I.n_entries > N * N + N) return "n_entries";
  const uint64_t nb = I.n_buckets, ne = im.n_records, T = (uint64_t)I.n_tiles;
  if (ne > I.n_entries / 2 + 32ull * T * nb + 64 || ne >= 0xFFFFFFFFull) return "n_records";
  return nullptr;
}

/* every (tile, bucket) in dealing order (position j = record 32*(j/64) + j%32, slot (j%64)/32): entries of low-half
 * rows, entries of high-half rows, padding -- what k_bucket_mid and the 32-bit passes of k_vote rely on */
bool image_halves_in_order(const ModelImage& im) {
  const uint64_t nb = im.info.n_buckets, T = (uint64_t)im.info.n_tiles;
  const uint32_t first_real = first_real_row(im.info.num_angles);
  for (uint64_t t = 0; t < T; t++)
    for (uint64_t b = 0; b < nb; b++) {
      const uint32_t off = im.bucket_off[t * (nb + 1) + b], cnt = im.bucket_off[t * (nb + 1) + b + 1] - off;
      int state = 0; /* 0: low halves, 1: high halves, 2: padding */
      for (uint32_t j = 0; j < 64u * ((cnt + 31u) / 32u); j++) {
        const uint32_t r = 32u * (j / 64u) + (j % 32u);
        if (r >= cnt) continue;
        const uint32_t code = (((j % 64u) / 32u) ? im.records[off + r].y : im.records[off + r].x) & ROW_CODE_MASK;
        const int kind = code < first_real ? 2 : (int)(code & 1u);
        if (kind < state) return false;
        state = kind;
      }
    }
  return true;
}

const char* image_body_fault(const ModelImage& im) {
  const ppf_model_info& I = im.info;
  const uint64_t nb = I.n_buckets, ne = im.n_records, T = (uint64_t)I.n_tiles;
  const int A = I.num_angles;
  for (float v : im.sampled)
    if (!std::isfinite(v)) return "sampled cloud";
  { /* slot map: ranks are the running popcount, which ends at n_buckets */
    uint64_t run = 0;
    for (const SlotWord& w : im.slotmap) {
      if (w.rank != run) return "slot map ranks";
      run += (uint64_t)__builtin_popcount(w.bits_lo) + (uint64_t)__builtin_popcount(w.bits_hi);
    }
    if (run != nb) return "slot map population";
  }
  for (uint32_t slot : im.bucket_slot)
    if (slot >= I.slots) return "bucket slots";
  { /* per-tile CSR rows over the records: monotone, chained tile to tile, ending at n_records */
    uint32_t prev = 0;
    for (uint64_t t = 0; t < T; t++) {
      const uint32_t* row = &im.bucket_off[t * (nb + 1)];
      if (row[0] != prev) return "bucket offsets (tile start)";
      for (uint64_t k = 0; k < nb; k++)
        if (row[k + 1] < row[k]) return "bucket offsets (order)";
      prev = row[nb];
    }
    if (prev != ne) return "bucket offsets (total)";
  }
  /* records: LDS byte offsets inside guard + the tile's word rows (a vote adds up to A*4 bytes) with the half of the
   * word in bit 0, finite alphas within (-pi, pi) */
  const uint32_t limit_words = (uint32_t)vote_lds_words(I.tile_refs, A);
  for (const uint4& rec : im.records) {
    const uint32_t codes[2] = {rec.x, rec.y}, al[2] = {rec.z, rec.w};
    for (int sl = 0; sl < 2; sl++) {
      const uint32_t row = codes[sl] & ROW_CODE_MASK, cx = (codes[sl] >> ROW_X_SHIFT) & 31u, cq = (codes[sl] >> ROW_Q_SHIFT) & ROW_Q_MASK;
      if ((row & 2u) || row / 4 + (uint32_t)A + 1 > limit_words) return "record row"; /* bin A of the last row: the word behind the rows */
      if ((codes[sl] >> 30) || cx > (uint32_t)A || cq > (uint32_t)AGG_Q) return "record cell";
      float av;
      memcpy(&av, &al[sl], 4);
      if (!(std::fabs(av) <= 3.1416f)) return "record alpha";
    }
  }
  return image_halves_in_order(im) ? nullptr : "record halves (order)";
}

/* A model file (or the same bytes in memory) into `im`, or PPF_ERR_IO with the check it failed.  The header is checked
 * before anything is sized from it.  Host only: no device, no ppf_model. */
ppf_status model_image_read(FILE* f, const char* path, ModelImage& im) {
  auto bad = [&](const char* what) { return fail(PPF_ERR_IO, "ppf_model_load: %s is not a valid model file (%s)", path, what); };
  if (fseek(f, 0, SEEK_END) != 0) return bad("seek");
  const long fsize = ftell(f);
  if (fsize < 0 || fseek(f, 0, SEEK_SET) != 0) return bad("seek");
  char magic[8];
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, PPF_MAGIC, 8) != 0) return bad("magic");
  ModelBuildWord bw;
  if (fread(&bw, sizeof(bw), 1, f) != 1) return bad("header");
  if (bw.agg_q != (uint32_t)AGG_Q || bw.reserved != 0u) return bad("written by a build with another count-table cell count");
  if (fread(&im.params, sizeof(im.params), 1, f) != 1 || fread(&im.info, sizeof(im.info), 1, f) != 1 ||
      fread(&im.n_records, sizeof(im.n_records), 1, f) != 1)
    return bad("header");
  if (const char* what = image_header_fault(im)) return bad(what);
  const ImageSections n = image_sections(im.info, im.n_records);
  if ((uint64_t)fsize != IMAGE_HEADER_BYTES + n.bytes()) return bad("file size does not match its header");
  im.sampled.resize(n.sampled);
  im.slotmap.resize(n.slotmap);
  im.bucket_off.resize(n.bucket_off);
  im.bucket_slot.resize(n.bucket_slot);
  im.records.resize(n.records);
  auto rd = [&](auto& v) { return v.empty() || fread(v.data(), sizeof(v[0]), v.size(), f) == v.size(); };
  if (!(rd(im.sampled) && rd(im.slotmap) && rd(im.bucket_off) && rd(im.bucket_slot) && rd(im.records))) return bad("short read");
  if (const char* what = image_body_fault(im)) return bad(what);
  return PPF_OK;
}
ppf_status model_image_read_path(const char* path, ModelImage& im) {
  FILE* f = fopen(path, "rb");
  if (!f) return fail(PPF_ERR_IO, "ppf_model_load: cannot open %s", path);
  Closer closer{f};
  return model_image_read(f, path, im);
}

/* the model as a byte stream (what a model file holds), written to an open FILE */
ppf_status model_image_write(const ModelImage& im, FILE* f, const char* path) {
  const ModelBuildWord bw = {(uint32_t)AGG_Q, 0u};
  auto wr = [&](const auto& v) { return fwrite(v.data(), sizeof(v[0]), v.size(), f) == v.size(); };
  bool ok = fwrite(PPF_MAGIC, 1, 8, f) == 8 && fwrite(&bw, sizeof(bw), 1, f) == 1;
  ok = ok && fwrite(&im.params, sizeof(im.params), 1, f) == 1 && fwrite(&im.info, sizeof(im.info), 1, f) == 1;
  ok = ok && fwrite(&im.n_records, sizeof(im.n_records), 1, f) == 1;
  ok = ok && wr(im.sampled) && wr(im.slotmap) && wr(im.bucket_off) && wr(im.bucket_slot) && wr(im.records);
  if (!ok) return fail(PPF_ERR_IO, "ppf_model_save: short write to %s", path);
  return PPF_OK;
}

/* device -> host: the header and the sections `parts` names (the others stay empty).  The only place with these copies. */
ppf_status model_download(const ppf_model* m, ModelImage& im, unsigned parts) {
  im.params = m->params;
  im.info = m->info;
  im.n_records = m->n_records;
  const ImageSections n = image_sections(m->info, m->n_records);
  auto down = [](auto& dst, const auto& src, uint64_t count) -> ppf_status {
    dst.resize(count);
    if (count) HIPCHK(hipMemcpy(dst.data(), src.p, count * sizeof(dst[0]), hipMemcpyDeviceToHost));
    return PPF_OK;
  };
  ppf_status s = PPF_OK;
  if (parts & IMG_SAMPLED) im.sampled = m->sampled;
  if (s == PPF_OK && (parts & IMG_SLOTMAP)) s = down(im.slotmap, m->slotmap, n.slotmap);
  if (s == PPF_OK && (parts & IMG_BUCKET_OFF)) s = down(im.bucket_off, m->bucket_off, n.bucket_off);
  if (s == PPF_OK && (parts & IMG_BUCKET_SLOT)) s = down(im.bucket_slot, m->bucket_slot, n.bucket_slot);
  if (s == PPF_OK && (parts & IMG_RECORDS)) s = down(im.records, m->records, n.records);
  return s;
}

/* host -> device: a whole image into a fresh model, ready for model_finish */
ppf_status model_upload(const ModelImage& im, ppf_model* m) {
  m->params = im.params;
  m->info = im.info;
  m->n_records = im.n_records;
  m->sampled = im.sampled;
  m->kd = key_lut_dims(im.params.feature, im.info.angle_step);
  auto up = [](auto& dst, const auto& src) -> ppf_status {
    HIPCHK(dst.reserve(std::max<size_t>(src.size(), 1)));
    if (!src.empty()) HIPCHK(hipMemcpy(dst.p, src.data(), src.size() * sizeof(src[0]), hipMemcpyHostToDevice));
    return PPF_OK;
  };
  ppf_status s = m->cloud.load_host(m->sampled.data(), im.info.n_ref, nullptr);
  if (s == PPF_OK) s = up(m->slotmap, im.slotmap);
  if (s == PPF_OK) s = up(m->bucket_off, im.bucket_off);
  if (s == PPF_OK) s = up(m->bucket_slot, im.bucket_slot);
  if (s == PPF_OK) s = up(m->records, im.records);
  return s;
}

/* ---- group records ---------------------------------------------------------------------------------- */
/* Group records: a second, (row, X)-sorted view of every (tile, bucket) that can vote through count tables (at least
 * PPF_AGG_MIN_RECORDS pair records).  The entries of a bucket that share accumulator row, half and count-table shift X cast
 * their counted adds at the same words and differ only in the table row T[q] they take the counts from, so k_vote adds up
 * the rows of up to AGG_GROUP_CELLS of them and casts one set of adds (agg_group_pair).  A group record is
 * {row code without its cell, cell bytes}: two of them make one 16-byte record {row_a, row_b, cells_a, cells_b}, laid out by
 * dealing position like the pair records (position j = record 32*(j/64) + j%32, slot (j%64)/32); a group of g entries
 * becomes ceil(g / AGG_GROUP_CELLS) records, a free slot names the all-zero row AGG_Q.  Every slot of the bucket's pair
 * records is an entry here, its padding included: the votes cast stay hits x slots.  Order inside a bucket: records with
 * more used slots first (a wave then reads the same number of rows in every lane), and inside such a class dealt over the
 * LDS banks like the entries (bank = (row word + X) mod DEAL_BANKS, every bank's records spread evenly over the class).
 * The records of a bucket are shared out over its chunks of AGG_CHUNK pair records in whole blocks of 32, in proportion to
 * the chunks' sizes; grp_hdr[first pair record of the chunk / 32] = {first group record, group records}.  Chunks of at least
 * 32 records start in different blocks of 32, and a smaller one (a bucket's last) gets no slice.
 * Derived from the pair records alone (like bucket_mid), on the host, once per model: not part of the model file. */
struct RowGroups {
  std::vector<std::vector<uint4>> pieces; /* the records: these, one behind the other (never joined on the host: a table of 10^6 pairs has 60 MB of them) */
  std::vector<uint2> hdr;                 /* n_records / 32 + 1, or empty: the model votes through no count table */
  size_t n_records = 0;
};
struct GroupSlice { uint32_t hdr, first, count; };
struct GroupPart { std::vector<uint4> out; std::vector<GroupSlice> slices; bool failed = false; };
struct Group { uint32_t code, cells, used; };
struct GroupScratch {
  std::vector<uint64_t> ent;
  std::vector<Group> grp;
  std::vector<std::pair<uint32_t, uint32_t>> order; /* {spread key, index} */
};

/* the groups of one bucket: its record slots sorted by (row, X), cut into runs of up to AGG_GROUP_CELLS cells */
void bucket_groups(const uint4* rec, uint32_t cnt, GroupScratch& S) {
  S.ent.clear();
  for (uint32_t r = 0; r < cnt; r++) {
    const uint32_t codes[2] = {rec[r].x, rec[r].y};
    for (int sl = 0; sl < 2; sl++)
      S.ent.push_back(((uint64_t)(codes[sl] & ((1u << ROW_Q_SHIFT) - 1u)) << 8) | ((codes[sl] >> ROW_Q_SHIFT) & ROW_Q_MASK));
  }
  std::sort(S.ent.begin(), S.ent.end());
  S.grp.clear();
  for (size_t i = 0; i < S.ent.size();) {
    size_t e = i;
    while (e < S.ent.size() && (S.ent[e] >> 8) == (S.ent[i] >> 8)) e++;
    for (size_t f = i; f < e; f += AGG_GROUP_CELLS) {
      Group g{(uint32_t)(S.ent[f] >> 8), AGG_CELLS_FREE, (uint32_t)std::min<size_t>(AGG_GROUP_CELLS, e - f)};
      for (uint32_t k = 0; k < g.used; k++) g.cells = (g.cells & ~(0xFFu << (8 * k))) | ((uint32_t)(S.ent[f + k] & 0xFFu) << (8 * k));
      S.grp.push_back(g);
    }
    i = e;
  }
}

/* the bucket's groups into n_rec group records at out[base ..]: free slots first, then the groups in dealing order */
void place_groups(GroupScratch& S, std::vector<uint4>& out, uint32_t base, uint32_t n_rec) {
  const uint32_t n_grp = (uint32_t)S.grp.size();
  for (uint32_t r = 0; r < n_rec; r++) {
    const uint32_t pad = ((base + r) & 63u) * 4u | (AGG_GROUP_X << ROW_X_SHIFT);
    out[base + r] = make_uint4(pad, pad, AGG_CELLS_FREE, AGG_CELLS_FREE);
  }
  uint32_t pos = 0;
  for (uint32_t used = AGG_GROUP_CELLS; used >= 1; used--) {
    uint32_t bank_n[DEAL_BANKS] = {0}, bank_k[DEAL_BANKS] = {0};
    auto bank = [](const Group& g) { return ((g.code & ROW_OFFSET_MASK) / 4u + ((g.code >> ROW_X_SHIFT) & 31u)) & (DEAL_BANKS - 1u); };
    for (const Group& g : S.grp) if (g.used == used) bank_n[bank(g)]++;
    S.order.clear();
    for (uint32_t i = 0; i < n_grp; i++)
      if (S.grp[i].used == used) {
        const uint32_t c = bank(S.grp[i]);
        S.order.emplace_back((uint32_t)((((uint64_t)(2u * bank_k[c] + 1u)) << 31) / bank_n[c]), i);
        bank_k[c]++;
      }
    std::stable_sort(S.order.begin(), S.order.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    for (const auto& o : S.order) {
      uint32_t* dst = reinterpret_cast<uint32_t*>(&out[base + 32u * (pos / 64u) + (pos % 32u)]);
      const uint32_t slot = (pos % 64u) / 32u;
      dst[slot] = S.grp[o.second].code;
      dst[2 + slot] = S.grp[o.second].cells;
      pos++;
    }
  }
}

/* the chunks of a bucket (cnt pair records from off) that take a slice of its n_rec group records, and their shares in
 * blocks of 32 records */
void chunk_slices(uint32_t off, uint32_t cnt, uint32_t base, uint32_t n_rec, std::vector<GroupSlice>& slices) {
  const uint32_t n_chunk = (cnt + AGG_CHUNK - 1) / AGG_CHUNK, blocks = (n_rec + 31u) / 32u;
  uint64_t elig = 0, cum = 0;
  for (uint32_t k = 0; k < n_chunk; k++) { const uint32_t c = std::min<uint32_t>(AGG_CHUNK, cnt - k * AGG_CHUNK); if (c >= 32u) elig += c; }
  for (uint32_t k = 0; k < n_chunk; k++) {
    const uint32_t c = std::min<uint32_t>(AGG_CHUNK, cnt - k * AGG_CHUNK);
    if (c < 32u) continue;
    const uint32_t b0 = (uint32_t)((uint64_t)blocks * cum / elig), b1 = (uint32_t)((uint64_t)blocks * (cum + c) / elig);
    cum += c;
    const uint32_t first = std::min(b0 * 32u, n_rec), end = std::min(b1 * 32u, n_rec);
    slices.push_back(GroupSlice{(off + k * (uint32_t)AGG_CHUNK) >> 5, base + first, end - first});
  }
}

/* whether k_vote can take this model's buckets through count tables at all */
bool has_count_tables(const ppf_model_info& I, uint64_t n_records) { return I.num_angles <= AGG_MAX_ANGLES && n_records && I.n_buckets; }

/* A pure function of the table (no device, no ppf_model).  Up to 8 threads share the buckets out by record offset and
 * their parts are joined in (tile, bucket) order. */
ppf_status row_groups(const std::vector<uint32_t>& boff, const std::vector<uint4>& rec, size_t nb, size_t T, int num_angles, RowGroups& out) {
  out = RowGroups{};
  const size_t nr = rec.size();
  if (num_angles > AGG_MAX_ANGLES || !nr || !nb) return PPF_OK; /* no count tables */
  const unsigned W = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  std::vector<GroupPart> parts(W);
  auto work = [&](unsigned w) {
    GroupPart& P = parts[w];
    try {
      GroupScratch S;
      for (size_t t = 0; t < T; t++)
        for (size_t b = 0; b < nb; b++) {
          const uint32_t off = boff[t * (nb + 1) + b], cnt = boff[t * (nb + 1) + b + 1] - off;
          if (cnt < (uint32_t)PPF_AGG_MIN_RECORDS || (unsigned)(((uint64_t)off * W) / nr) != w) continue;
          bucket_groups(&rec[off], cnt, S);
          const uint32_t n_rec = records_for((uint32_t)S.grp.size()), base = (uint32_t)P.out.size();
          P.out.resize((size_t)base + n_rec);
          place_groups(S, P.out, base, n_rec);
          chunk_slices(off, cnt, base, n_rec, P.slices);
        }
    } catch (...) {
      P.failed = true;
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned w = 1; w < W; w++) th.emplace_back(work, w);
    work(0);
    for (auto& x : th) x.join();
  }
  size_t total = 0;
  for (const GroupPart& P : parts) {
    if (P.failed) return fail(PPF_ERR_NOMEM, "ppf_model: out of host memory building the group records");
    total += P.out.size();
  }
  if (total >= 0xFFFFFFFFull) return fail(PPF_ERR_INVALID, "ppf_model: %zu group records are more than 32 bits index", total);
  out.hdr.assign((nr >> 5) + 1, make_uint2(0u, 0u));
  for (GroupPart& P : parts) {
    for (const auto& sl : P.slices) out.hdr[sl.hdr] = make_uint2((uint32_t)(out.n_records + sl.first), sl.count);
    out.n_records += P.out.size();
    out.pieces.push_back(std::move(P.out));
  }
  return PPF_OK;
}

/* ---- what is derived once the table stands ---------------------------------------------------------- */
ppf_status build_key_lut(ppf_model* m, hipStream_t st) {
  const size_t n = key_table_size(m->kd);
  HIPCHK(m->key_lut.reserve(n));
  k_build_key_lut<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(m->slotmap.p, m->info.slots - 1, m->params.key_equality == PPF_KEY_EXACT,
                                                                           m->kd, m->key_lut.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return PPF_OK;
}

/* bucket_total, bucket_mid, the key LUT, the group records and device_bytes: none of them is in the model file.  `host`
 * is the table on the host when the caller has it (loading); training has not, and downloads the two arrays the group
 * records are made from. */
ppf_status model_finish(ppf_model* m, hipStream_t st, const ModelImage* host) {
  const uint32_t nb = m->info.n_buckets;
  const int T = m->info.n_tiles;
  HIPCHK(m->bucket_total.reserve(std::max<uint32_t>(nb, 1)));
  if (nb) {
    k_bucket_total<<<dim3((nb + 255) / 256), dim3(256), 0, st>>>(m->bucket_off.p, (int)nb, T, m->bucket_total.p);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(m->bucket_mid.reserve(std::max<size_t>((size_t)nb * T, 1)));
  if (nb) {
    k_bucket_mid<<<dim3((unsigned)(((size_t)nb * T + 255) / 256)), dim3(256), 0, st>>>(
        m->bucket_off.p, (int)nb, T, m->records.p, first_real_row(m->info.num_angles), m->bucket_mid.p);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));
  ppf_status s = build_key_lut(m, st);
  if (s != PPF_OK) return s;
  if (has_count_tables(m->info, m->n_records)) {
    ModelImage mine;
    if (!host) {
      s = model_download(m, mine, IMG_BUCKET_OFF | IMG_RECORDS);
      if (s != PPF_OK) return s;
      host = &mine;
    }
    RowGroups rg;
    s = row_groups(host->bucket_off, host->records, nb, (size_t)T, m->info.num_angles, rg);
    if (s != PPF_OK) return s;
    HIPCHK(m->grp_records.reserve(std::max<size_t>(rg.n_records, 1)));
    HIPCHK(m->grp_hdr.reserve(rg.hdr.size()));
    size_t base = 0;
    for (const auto& piece : rg.pieces) {
      if (!piece.empty()) HIPCHK(hipMemcpy(m->grp_records.p + base, piece.data(), piece.size() * sizeof(uint4), hipMemcpyHostToDevice));
      base += piece.size();
    }
    HIPCHK(hipMemcpy(m->grp_hdr.p, rg.hdr.data(), rg.hdr.size() * sizeof(uint2), hipMemcpyHostToDevice));
    m->n_grp_records = rg.n_records;
  }
  m->info.device_bytes = m->cloud.buf.bytes() + m->slotmap.bytes() + m->bucket_off.bytes() + m->bucket_slot.bytes() +
                         m->records.bytes() + m->key_lut.bytes() + m->grp_records.bytes() + m->grp_hdr.bytes();
  return PPF_OK;
}

/* ---- training: the table build ------------------------------------------------------------------------ */
/* the temporaries of one table build; they live until build_table returns (the sort scratch of train_positions does not) */
struct TrainScratch {
  static constexpr int levels = 2; /* dealing levels: the accumulator-word half of the entry's row */
  int N = 0;
  size_t NN = 0, words = 0, ncnt = 0; /* pairs, slot-map words, (tile, bucket) counters + 1 */
  unsigned nblk = 0;                  /* blocks of 256 pairs */
  uint32_t n_buckets = 0, gmax = 0;   /* gmax: cell groups of a level at most */
  DevBuf<uint32_t> pair_slot, word_cnt, word_rank, counts, offsets, rec_cnt, level_cnt, mirror_cur, group_cnt;
  DevBuf<float> pair_alpha;
  DevBuf<unsigned long long> bits;
  DevBuf<uint32_t> pair_pos; /* dealing position of every pair inside its (tile, bucket, level, cell group) */
};

/* buckets: every pair's slot and alpha, the bit set of the slots in use, the slot map and n_buckets */
ppf_status train_buckets(ppf_model* m, TrainScratch& S, hipStream_t st) {
  const int N = S.N = m->info.n_ref;
  S.NN = (size_t)N * N;
  S.nblk = (unsigned)((S.NN + 255) / 256);
  const uint32_t slots = m->info.slots;
  const size_t words = S.words = (slots + 63) / 64;
  HIPCHK(S.pair_slot.reserve(S.NN));
  HIPCHK(S.pair_alpha.reserve(S.NN));
  HIPCHK(S.bits.reserve(words));
  HIPCHK(hipMemsetAsync(S.bits.p, 0, words * sizeof(unsigned long long), st));
  k_train_pairs<<<dim3(N), dim3(256), 0, st>>>(m->cloud.view(), m->info.angle_step, m->info.distance_step, slots - 1,
                                               m->params.key_equality == PPF_KEY_EXACT, m->params.feature == PPF_FEATURE_DARBOUX, m->kd,
                                               S.pair_slot.p, S.pair_alpha.p, S.bits.p);
  HIPCHK(hipGetLastError());
  HIPCHK(S.word_cnt.reserve(words + 1));
  HIPCHK(S.word_rank.reserve(words + 1));
  HIPCHK(hipMemsetAsync(S.word_cnt.p, 0, (words + 1) * sizeof(uint32_t), st));
  k_popcount_words<<<dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st>>>(S.bits.p, S.word_cnt.p, words);
  HIPCHK(hipGetLastError());
  ppf_status s = device_exclusive_scan(S.word_cnt.p, S.word_rank.p, words + 1, st);
  if (s != PPF_OK) return s;
  HIPCHK(hipMemcpyAsync(&S.n_buckets, S.word_rank.p + words, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  m->info.n_buckets = S.n_buckets;
  HIPCHK(m->slotmap.reserve(words));
  k_pack_slotmap<<<dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st>>>(S.bits.p, S.word_rank.p, m->slotmap.p, words);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

/* counts: the count pass of k_train_bin, the scans of entries and of records, bucket_off, the records initialised */
ppf_status train_counts(ppf_model* m, TrainScratch& S, hipStream_t st) {
  const int T = m->info.n_tiles, levels = TrainScratch::levels;
  const uint32_t n_buckets = S.n_buckets;
  const size_t ncnt = S.ncnt = (size_t)T * n_buckets + 1;
  HIPCHK(S.counts.reserve(ncnt));
  HIPCHK(S.rec_cnt.reserve(ncnt));
  HIPCHK(S.offsets.reserve(ncnt));
  HIPCHK(m->bucket_slot.reserve(std::max<uint32_t>(n_buckets, 1)));
  HIPCHK(hipMemsetAsync(S.counts.p, 0, ncnt * sizeof(uint32_t), st));
  /* Dealing order inside a bucket (see "table layout" above): two levels (the accumulator-word half of the entry's row),
   * a level cut into up to gmax cell groups, inside a group every bank's entries in phase order, spread evenly over it. */
  uint32_t gmax = (uint32_t)AGG_Q; /* one group per count-table cell at most; fewer groups when the class keys would not fit 32 bits or the group counters would be unreasonably big */
  while (gmax > 1 && (ncnt * (size_t)levels * gmax * DEAL_BANKS >= 0xFFFFFFF0ull || ncnt * (size_t)levels * gmax * sizeof(uint32_t) > ((size_t)1 << 30)))
    gmax >>= 1;
  if (ncnt * (size_t)levels * gmax * DEAL_BANKS >= 0xFFFFFFF0ull)
    return fail(PPF_ERR_INVALID, "ppf_model_train: %u buckets x %d tiles are more than the table build can key", n_buckets, T);
  S.gmax = gmax;
  HIPCHK(S.level_cnt.reserve(ncnt * levels));
  HIPCHK(S.mirror_cur.reserve(ncnt));
  HIPCHK(S.group_cnt.reserve(ncnt * levels * gmax));
  HIPCHK(hipMemsetAsync(S.level_cnt.p, 0, ncnt * levels * sizeof(uint32_t), st));
  HIPCHK(hipMemsetAsync(S.mirror_cur.p, 0, ncnt * sizeof(uint32_t), st));
  HIPCHK(hipMemsetAsync(S.group_cnt.p, 0, ncnt * levels * gmax * sizeof(uint32_t), st));
  k_train_bin<<<dim3(S.nblk), dim3(256), 0, st>>>(S.pair_slot.p, S.pair_alpha.p, S.N, m->slotmap.p, (int)n_buckets,
                                                  m->info.tile_refs, T, m->info.num_angles, levels, S.counts.p, nullptr,
                                                  S.level_cnt.p, S.mirror_cur.p, nullptr, gmax, nullptr, m->bucket_slot.p, 0);
  HIPCHK(hipGetLastError());
  /* real entries (N(N-1) + mirrored spill entries) */
  ppf_status s = device_exclusive_scan(S.counts.p, S.offsets.p, ncnt, st);
  if (s != PPF_OK) return s;
  uint32_t n_entries = 0;
  HIPCHK(hipMemcpyAsync(&n_entries, S.offsets.p + (ncnt - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  /* record offsets */
  k_record_counts<<<dim3((unsigned)((ncnt + 255) / 256)), dim3(256), 0, st>>>(S.counts.p, S.rec_cnt.p, ncnt - 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(S.rec_cnt.p + (ncnt - 1), 0, sizeof(uint32_t), st));
  s = device_exclusive_scan(S.rec_cnt.p, S.offsets.p, ncnt, st);
  if (s != PPF_OK) return s;
  uint32_t n_records = 0;
  HIPCHK(hipMemcpyAsync(&n_records, S.offsets.p + (ncnt - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  m->info.n_entries = n_entries;
  m->n_records = n_records;
  /* per-tile CSR rows of n_buckets+1 RECORD offsets: row t = offsets[t*NB .. t*NB+NB] (the next row's first
   * element closes the last bucket), materialised with an explicit copy per tile */
  HIPCHK(m->bucket_off.reserve((size_t)T * (n_buckets + 1)));
  for (int t = 0; t < T; t++)
    HIPCHK(hipMemcpyAsync(m->bucket_off.p + (size_t)t * (n_buckets + 1), S.offsets.p + (size_t)t * n_buckets,
                          (size_t)(n_buckets + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(m->records.reserve(std::max<uint32_t>(n_records, 1)));
  if (n_records) {
    k_record_init<<<dim3((n_records + 255) / 256), dim3(256), 0, st>>>(m->records.p, n_records, m->info.num_angles);
    HIPCHK(hipGetLastError());
  }
  return PPF_OK;
}

/* the second of two chained sorts: the values come from whichever of v1 / v2 the first sort left them in (*va) */
ppf_status sort_again(DevBuf<uint32_t>& keys, DevBuf<uint32_t>& v1, DevBuf<uint32_t>& keys2, DevBuf<uint32_t>& v2, size_t n,
                      unsigned long long max_key, DevBuf<uint32_t>& starts, uint32_t** va, uint32_t* n_runs, hipStream_t st) {
  const bool in1 = *va == v1.p;
  return sort_segments(keys, in1 ? v1 : v2, keys2, in1 ? v2 : v1, (int)n, max_key, starts, va, n_runs, st);
}

/* dealing positions: four sorts give every pair its position inside its (tile, bucket, level, cell group) */
ppf_status train_positions(ppf_model* m, TrainScratch& S, hipStream_t st) {
  const size_t NN = S.NN;
  const unsigned nblk = S.nblk;
  DevBuf<uint32_t> kcls, kph, v1, kt, v2, starts, pair_rank, pair_n;
  HIPCHK(kcls.reserve(NN)); HIPCHK(kph.reserve(NN)); HIPCHK(v1.reserve(NN)); HIPCHK(kt.reserve(NN)); HIPCHK(v2.reserve(NN));
  HIPCHK(pair_rank.reserve(NN)); HIPCHK(pair_n.reserve(NN)); HIPCHK(S.pair_pos.reserve(NN));
  const uint32_t invalid = (uint32_t)((size_t)m->info.n_tiles * S.n_buckets * 2 * S.gmax * DEAL_BANKS);
  k_train_keys<<<dim3(nblk), dim3(256), 0, st>>>(S.pair_slot.p, S.pair_alpha.p, S.N, m->slotmap.p, (int)S.n_buckets, m->info.tile_refs,
                                                 m->info.num_angles, S.level_cnt.p, S.gmax, S.group_cnt.p, invalid, kcls.p, kph.p, v1.p);
  HIPCHK(hipGetLastError());
  /* (1) rank of every pair by phase inside its (tile, bucket, level, bank): two stable sorts (phase, then group) */
  uint32_t* va = nullptr;
  uint32_t n_runs = 0;
  ppf_status s = sort_segments(kph, v1, kt, v2, (int)NN, 65535ull, starts, &va, &n_runs, st);
  if (s != PPF_OK) return s;
  k_gather_u32<<<dim3(nblk), dim3(256), 0, st>>>(kcls.p, va, NN, kph.p); /* group keys in phase order */
  HIPCHK(hipGetLastError());
  s = sort_again(kph, v1, kt, v2, NN, (unsigned long long)invalid, starts, &va, &n_runs, st);
  if (s != PPF_OK) return s;
  k_train_ranks<<<dim3(nblk), dim3(256), 0, st>>>(va, starts.p, n_runs, NN, pair_rank.p, pair_n.p);
  HIPCHK(hipGetLastError());
  /* (2) position inside the cell group: the banks' entries spread evenly, i.e. sorted by (rank + 1/2) / class size; ties keep
   * the pair order (stable sorts from the identity) */
  k_train_spread<<<dim3(nblk), dim3(256), 0, st>>>(kcls.p, pair_rank.p, pair_n.p, invalid, NN, kph.p, kt.p, v1.p);
  HIPCHK(hipGetLastError());
  DevBuf<uint32_t> kseg;
  HIPCHK(kseg.reserve(NN));
  HIPCHK(hipMemcpyAsync(kseg.p, kt.p, NN * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  s = sort_segments(kph, v1, kt, v2, (int)NN, 0xFFFFFFFFull, starts, &va, &n_runs, st);
  if (s != PPF_OK) return s;
  k_gather_u32<<<dim3(nblk), dim3(256), 0, st>>>(kseg.p, va, NN, kph.p); /* level keys in fraction order */
  HIPCHK(hipGetLastError());
  s = sort_again(kph, v1, kt, v2, NN, (unsigned long long)(invalid / DEAL_BANKS), starts, &va, &n_runs, st);
  if (s != PPF_OK) return s;
  k_train_ranks<<<dim3(nblk), dim3(256), 0, st>>>(va, starts.p, n_runs, NN, S.pair_pos.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st)); /* the sort scratch dies here */
  return PPF_OK;
}

/* fill: the place pass of k_train_bin writes every entry into its record slot */
ppf_status train_fill(ppf_model* m, TrainScratch& S, hipStream_t st) {
  k_train_bin<<<dim3(S.nblk), dim3(256), 0, st>>>(S.pair_slot.p, S.pair_alpha.p, S.N, m->slotmap.p, (int)S.n_buckets,
                                                  m->info.tile_refs, m->info.n_tiles, m->info.num_angles, TrainScratch::levels, S.counts.p, S.offsets.p,
                                                  S.level_cnt.p, S.mirror_cur.p, S.group_cnt.p, S.gmax, m->records.p, nullptr, 1, S.pair_pos.p);
  HIPCHK(hipGetLastError());
  return PPF_OK;
}

ppf_status build_table(ppf_model* m, hipStream_t st) {
  TrainScratch S;
  ppf_status s = train_buckets(m, S, st);
  if (s == PPF_OK) s = train_counts(m, S, st);
  if (s == PPF_OK) s = train_positions(m, S, st);
  if (s == PPF_OK) s = train_fill(m, S, st);
  if (s == PPF_OK) s = model_finish(m, st, nullptr);
  return s;
}

/* the model cloud's sampled rows on the device (m->cloud) and on the host (m->sampled) */
ppf_status train_sample(ppf_model* m, const float* xyzn, int n, int stride, int noff, hipStream_t st) {
  if (m->params.presampled) {
    m->sampled.resize((size_t)n * 6);
    for (int i = 0; i < n; i++) {
      memcpy(&m->sampled[(size_t)i * 6], xyzn + (size_t)i * stride, 12);
      memcpy(&m->sampled[(size_t)i * 6 + 3], xyzn + (size_t)i * stride + noff, 12);
    }
    return m->cloud.load_host(m->sampled.data(), n, st);
  }
  /* A2 on the device: upload the raw model cloud, sample, keep a host copy of the sampled rows */
  DevBuf<float> d_raw;
  hipError_t e = d_raw.reserve((size_t)n * stride);
  if (e == hipSuccess) e = hipMemcpy(d_raw.p, xyzn, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(PPF_ERR_HIP, "ppf_model_train: upload failed: %s", hipGetErrorString(e));
  return device_sample_cloud(d_raw.p, n, stride, noff, (float)m->params.relative_sampling_step, m->cloud, &m->sampled, st);
}

/* ---- loading and saving --------------------------------------------------------------------------------- */
/* a validated image -> a model on the current device */
ppf_status model_from_image(const ModelImage& im, ppf_model** out) {
  std::unique_ptr<ppf_model> owner(new ppf_model()); /* released on every early return */
  ppf_model* m = owner.get();
  HIPCHK(hipGetDevice(&m->device));
  ppf_status s = model_upload(im, m);
  if (s == PPF_OK) s = model_finish(m, nullptr, &im);
  if (s != PPF_OK) return s;
  *out = owner.release();
  return PPF_OK;
}
ppf_status model_save_stream(const ppf_model* m, FILE* f, const char* path) {
  ModelImage im;
  ppf_status s = model_download(m, im, IMG_ALL);
  return s != PPF_OK ? s : model_image_write(im, f, path);
}

/* No exception leaves a file entry: what reading a file (or its bytes, path == NULL) throws becomes a status. */
template <class F>
ppf_status guarded(const char* entry, const char* path, F fn) {
  try {
    return fn();
  } catch (const std::bad_alloc&) {
    return path ? fail(PPF_ERR_NOMEM, "%s: out of host memory reading %s", entry, path) : fail(PPF_ERR_NOMEM, "%s: out of host memory", entry);
  } catch (...) {
    return path ? fail(PPF_ERR_IO, "%s: %s is not a valid model file", entry, path) : fail(PPF_ERR_IO, "%s: not a valid model", entry);
  }
}

}  // namespace

extern "C" {

ppf_status ppf_model_train(const float* xyzn, int n, int stride, int noff, const ppf_train_params* params, ppf_model** out) {
  if (!out) return fail(PPF_ERR_INVALID, "ppf_model_train: out is NULL");
  *out = nullptr;
  if (!xyzn || n <= 1 || bad_layout(stride, noff) || !params) return fail(PPF_ERR_INVALID, "ppf_model_train: bad argument");
  if (!(params->relative_sampling_step > 0) || !(params->num_angles >= 1))
    return fail(PPF_ERR_INVALID, "ppf_model_train: bad parameters");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_model_train: no HIP device (this engine has no CPU fallback)");
  std::unique_ptr<ppf_model> owner(new ppf_model()); /* released on every early return */
  ppf_model* m = owner.get();
  m->params = *params;
  HIPCHK(hipGetDevice(&m->device));
  float lo[3], hi[3];
  bbox_host(xyzn, n, stride, lo, hi);
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  const float diameter = std::sqrt(dx * dx + dy * dy + dz * dz);
  hipStream_t st = nullptr;
  ppf_status s = train_sample(m, xyzn, n, stride, noff, st);
  if (s != PPF_OK) return s;
  ModelPlan plan;
  s = model_plan((int)(m->sampled.size() / 6), diameter, *params, plan);
  if (s != PPF_OK) return s;
  m->info = plan.info;
  m->kd = plan.kd;
  s = build_table(m, st);
  if (s != PPF_OK) return s;
  *out = owner.release();
  return PPF_OK;
}

ppf_status ppf_pair_features(const float* xyzn, int n, int stride, int noff, int feature, float* out, size_t cap_rows) {
  if (!xyzn || n <= 0 || bad_layout(stride, noff) || !out || (feature != PPF_FEATURE_PPF && feature != PPF_FEATURE_DARBOUX))
    return fail(PPF_ERR_INVALID, "ppf_pair_features: bad argument");
  const size_t rows = (size_t)n * (size_t)n;
  if (cap_rows < rows) return fail(PPF_ERR_CAPACITY, "ppf_pair_features: need room for %zu rows", rows);
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_pair_features: no HIP device (this engine has no CPU fallback)");
  DevBuf<float> d_raw, d_out;
  CloudDev cloud;
  HIPCHK(d_raw.reserve((size_t)n * stride));
  HIPCHK(hipMemcpy(d_raw.p, xyzn, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice));
  ppf_status s = cloud.load_device(d_raw.p, n, stride, noff, nullptr);
  if (s != PPF_OK) return s;
  HIPCHK(d_out.reserve(rows * 5));
  k_pair_features<<<dim3((unsigned)n), dim3(256)>>>(cloud.view(), feature == PPF_FEATURE_DARBOUX ? 1 : 0, d_out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, d_out.p, rows * 5 * sizeof(float), hipMemcpyDeviceToHost));
  return PPF_OK;
}

ppf_status ppf_model_nearest_pairs(const ppf_model* m, const float* f4, uint32_t* pairs_ij, int cap_pairs, int* n_out) {
  if (!m || !f4 || !n_out || cap_pairs < 0 || (cap_pairs > 0 && !pairs_ij)) return fail(PPF_ERR_INVALID, "ppf_model_nearest_pairs: bad argument");
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_model_nearest_pairs: no HIP device (this engine has no CPU fallback)");
  const bool darboux = m->params.feature == PPF_FEATURE_DARBOUX;
  const double as = m->info.angle_step, ds = m->info.distance_step;
  int32_t k[4];
  for (int c = 0; c < 4; c++) { /* the key of the query: the quantisation the table's pairs went through */
    const double q = (double)f4[c] / (c < 3 ? as : ds);
    k[c] = darboux ? ppf_floor_key(q) : ppf_d2i(q);
  }
  const int n = m->info.n_ref;
  DevBuf<uint2> d_out;
  DevBuf<uint32_t> d_cur;
  const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)n * (uint64_t)n, 1u << 26); /* 512 MB at most */
  HIPCHK(d_out.reserve(std::max<uint32_t>(cap, 1u)));
  HIPCHK(d_cur.reserve(1));
  HIPCHK(hipMemset(d_cur.p, 0, sizeof(uint32_t)));
  k_key_pairs<<<dim3((unsigned)n), dim3(256)>>>(m->cloud.view(), darboux ? 1 : 0, as, ds, k[0], k[1], k[2], k[3], d_out.p, cap, d_cur.p);
  HIPCHK(hipGetLastError());
  uint32_t found = 0;
  HIPCHK(hipMemcpy(&found, d_cur.p, sizeof(found), hipMemcpyDeviceToHost));
  if (found > cap) return fail(PPF_ERR_CAPACITY, "ppf_model_nearest_pairs: %u pairs share this key, more than one call returns", found);
  *n_out = (int)found;
  if ((int)found > cap_pairs) return cap_pairs == 0 ? PPF_OK : fail(PPF_ERR_CAPACITY, "ppf_model_nearest_pairs: need room for %u pairs", found);
  std::vector<uint2> h(found);
  if (found) HIPCHK(hipMemcpy(h.data(), d_out.p, (size_t)found * sizeof(uint2), hipMemcpyDeviceToHost));
  std::sort(h.begin(), h.end(), [](const uint2& a, const uint2& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
  for (uint32_t q = 0; q < found; q++) { pairs_ij[2 * q] = h[q].x; pairs_ij[2 * q + 1] = h[q].y; }
  return PPF_OK;
}

ppf_status ppf_model_retain(ppf_model* m) {
  if (!m) return fail(PPF_ERR_INVALID, "ppf_model_retain: NULL");
  m->refcount.fetch_add(1);
  return PPF_OK;
}
ppf_status ppf_model_release(ppf_model* m) {
  if (!m) return PPF_OK;
  if (m->refcount.fetch_sub(1) == 1) {
    sync_device(m->device); /* the table returns to the block cache: no match may still be reading it */
    delete m;
  }
  return PPF_OK;
}
ppf_status ppf_model_get_info(const ppf_model* m, ppf_model_info* info) {
  if (!m || !info) return fail(PPF_ERR_INVALID, "ppf_model_get_info: NULL");
  *info = m->info;
  return PPF_OK;
}
ppf_status ppf_model_get_device(const ppf_model* m, int* device) {
  if (!m || !device) return fail(PPF_ERR_INVALID, "ppf_model_get_device: NULL");
  *device = m->device;
  return PPF_OK;
}
ppf_status ppf_model_get_sampled(const ppf_model* m, float* out, int cap_rows) {
  if (!m || !out) return fail(PPF_ERR_INVALID, "ppf_model_get_sampled: NULL");
  if (cap_rows < m->info.n_ref) return fail(PPF_ERR_CAPACITY, "ppf_model_get_sampled: need %d rows", m->info.n_ref);
  memcpy(out, m->sampled.data(), m->sampled.size() * sizeof(float));
  return PPF_OK;
}
ppf_status ppf_model_get_table(const ppf_model* m, uint32_t* bucket_slot, uint32_t* bucket_off, int32_t* entry_cell,
                               float* entry_alpha) {
  if (!m) return fail(PPF_ERR_INVALID, "ppf_model_get_table: NULL");
  const size_t nb = m->info.n_buckets;
  const int T = m->info.n_tiles, A = m->info.num_angles;
  const bool decode = bucket_off || entry_cell || entry_alpha;
  ModelImage im;
  ppf_status s = model_download(m, im, (bucket_slot ? IMG_BUCKET_SLOT : 0u) | (decode ? IMG_BUCKET_OFF | IMG_RECORDS : 0u));
  if (s != PPF_OK) return s;
  if (bucket_slot && nb) memcpy(bucket_slot, im.bucket_slot.data(), nb * sizeof(uint32_t));
  if (!decode) return PPF_OK;
  /* decode the pair records: per (tile, bucket) the real entries in storage order; dummies (row in the first
   * guard words) are skipped; the CSR handed out counts ENTRIES */
  const std::vector<uint32_t>& roff = im.bucket_off;
  const std::vector<uint4>& rec = im.records;
  const uint32_t first_real = first_real_row(A);
  size_t k = 0;
  for (int t = 0; t < T; t++) {
    for (size_t b = 0; b < nb; b++) {
      if (bucket_off) bucket_off[(size_t)t * (nb + 1) + b] = (uint32_t)k;
      for (uint32_t r = roff[(size_t)t * (nb + 1) + b]; r < roff[(size_t)t * (nb + 1) + b + 1]; r++) {
        const uint32_t rows[2] = {rec[r].x & ROW_CODE_MASK, rec[r].y & ROW_CODE_MASK}, al[2] = {rec[r].z, rec[r].w};
        for (int sl = 0; sl < 2; sl++) {
          if (rows[sl] < first_real) continue;
          if (k >= m->info.n_entries) return fail(PPF_ERR_INVALID, "ppf_model_get_table: more entries than counted");
          if (entry_cell) { /* byte offset of the row -> reference layout local_ref*numAngles (mirrored spill entries: -numAngles) */
            const int32_t w = (int32_t)(rows[sl] / 4) - vote_guard(A);
            entry_cell[k] = w < 0 ? -A : (w / vote_pitch(A) + (int32_t)(rows[sl] & 1u) * vote_half_rows(m->info.tile_refs)) * A;
          }
          if (entry_alpha) memcpy(&entry_alpha[k], &al[sl], 4);
          k++;
        }
      }
    }
    if (bucket_off) bucket_off[(size_t)t * (nb + 1) + nb] = (uint32_t)k;
  }
  return PPF_OK;
}

ppf_status ppf_model_save(const ppf_model* m, const char* path) {
  if (!m || !path) return fail(PPF_ERR_INVALID, "ppf_model_save: NULL");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(PPF_ERR_IO, "ppf_model_save: cannot open %s", path);
  ppf_status s = model_save_stream(m, f, path);
  if (fclose(f) != 0 && s == PPF_OK) s = fail(PPF_ERR_IO, "ppf_model_save: short write to %s", path);
  return s;
}

/* the same bytes into the caller's memory: no file in between (the FileStorage overloads of the C++ facade) */
ppf_status ppf_model_save_mem(const ppf_model* m, void* buf, size_t cap, size_t* size) {
  if (!m || !size) return fail(PPF_ERR_INVALID, "ppf_model_save_mem: NULL");
  char* mem = nullptr;
  size_t len = 0;
  FILE* f = open_memstream(&mem, &len);
  if (!f) return fail(PPF_ERR_NOMEM, "ppf_model_save_mem: out of memory");
  ppf_status s = model_save_stream(m, f, "memory");
  if (fclose(f) != 0 && s == PPF_OK) s = fail(PPF_ERR_NOMEM, "ppf_model_save_mem: out of memory");
  if (s == PPF_OK) {
    *size = len;
    if (buf && cap >= len) memcpy(buf, mem, len);
    else if (buf) s = fail(PPF_ERR_CAPACITY, "ppf_model_save_mem: need %zu bytes", len);
  }
  free(mem);
  return s;
}

ppf_status ppf_model_load(const char* path, ppf_model** out) {
  if (!path || !out) return fail(PPF_ERR_INVALID, "ppf_model_load: NULL");
  *out = nullptr;
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_model_load: no HIP device");
  return guarded("ppf_model_load", path, [&] {
    ModelImage im;
    const ppf_status s = model_image_read_path(path, im);
    return s != PPF_OK ? s : model_from_image(im, out);
  });
}

ppf_status ppf_model_load_mem(const void* buf, size_t size, ppf_model** out) {
  if (!buf || !out) return fail(PPF_ERR_INVALID, "ppf_model_load_mem: NULL");
  *out = nullptr;
  if (!have_device()) return fail(PPF_ERR_HIP, "ppf_model_load_mem: no HIP device");
  if (size == 0) return fail(PPF_ERR_IO, "ppf_model_load: memory is not a valid model file (empty)");
  FILE* f = fmemopen(const_cast<void*>(buf), size, "rb");
  if (!f) return fail(PPF_ERR_NOMEM, "ppf_model_load_mem: out of memory");
  Closer closer{f};
  return guarded("ppf_model_load_mem", nullptr, [&] {
    ModelImage im;
    const ppf_status s = model_image_read(f, "memory", im);
    return s != PPF_OK ? s : model_from_image(im, out);
  });
}

ppf_status ppf_model_check_file(const char* path) {
  if (!path) return fail(PPF_ERR_INVALID, "ppf_model_check_file: NULL");
  return guarded("ppf_model_check_file", path, [&] {
    ModelImage im;
    return model_image_read_path(path, im);
  });
}

ppf_status ppf_debug_model_row_groups(const void* model_bytes, size_t size, uint32_t* grp_records, size_t cap_records, uint32_t* grp_hdr,
                                      size_t cap_hdr, uint64_t* n_records_out, uint64_t* n_hdr_out) {
  if (!model_bytes || !n_records_out || !n_hdr_out) return fail(PPF_ERR_INVALID, "ppf_debug_model_row_groups: NULL");
  *n_records_out = *n_hdr_out = 0;
  if (size == 0) return fail(PPF_ERR_IO, "ppf_model_load: memory is not a valid model file (empty)");
  FILE* f = fmemopen(const_cast<void*>(model_bytes), size, "rb");
  if (!f) return fail(PPF_ERR_NOMEM, "ppf_debug_model_row_groups: out of memory");
  Closer closer{f};
  return guarded("ppf_debug_model_row_groups", nullptr, [&] {
    ModelImage im;
    RowGroups rg;
    ppf_status s = model_image_read(f, "memory", im);
    if (s == PPF_OK) s = row_groups(im.bucket_off, im.records, im.info.n_buckets, (size_t)im.info.n_tiles, im.info.num_angles, rg);
    if (s != PPF_OK) return s;
    *n_records_out = rg.n_records;
    *n_hdr_out = rg.hdr.size();
    if ((grp_records && cap_records < rg.n_records) || (grp_hdr && cap_hdr < rg.hdr.size()))
      return fail(PPF_ERR_CAPACITY, "ppf_debug_model_row_groups: need room for %zu group records and %zu header entries", rg.n_records, rg.hdr.size());
    for (const auto& piece : rg.pieces) {
      if (grp_records && !piece.empty()) memcpy(grp_records, piece.data(), piece.size() * sizeof(uint4));
      if (grp_records) grp_records += 4 * piece.size();
    }
    if (grp_hdr && !rg.hdr.empty()) memcpy(grp_hdr, rg.hdr.data(), rg.hdr.size() * sizeof(uint2));
    return PPF_OK;
  });
}

}  // extern "C"

#endif /* PPF_MODEL_HOST_H */
