// emu_csv_ws.cpp -- TEST INFRASTRUCTURE ONLY: CPU emulation of the single-pass
// CSV tile bodies added for whitespace delimiters and integer label columns
// (csv_fast.h tile<MODE, SP, VT, WS>).
//
// emu.cpp runs the instantiations it was written for and decides with the
// predicates of its time; this driver decides as capi.cpp does today (args.h
// csv_single_pass_delim / csv_single_pass_columns), runs the tile body that
// csv.hip's launch_fast_tile would launch, and hands everything else -- other
// formats, FLAG_EXACT, and an input that left the grammar -- to emu.cpp's
// emu_parse on its exact path.  Same command line and output files as emu.cpp.
#define main emu_base_main
#include "emu.cpp"
#undef main

namespace {

// one single-pass tile, as launch_fast_tile (csv.hip) picks the kernel
template <int MODE>
void run_fast_tile(const FastCsvArgs &f, fcsv::Shared &sh, uint32_t k) {
  const bool sp = f.label_col >= 0 || f.weight_col >= 0, iv = f.vtype != 0, ws = f.ws != 0;
#define EMU_GO(SP, VT, WS) \
  return run_block<fast::kFThreads>([&](FastBlock &bk) { fcsv::tile<MODE, SP, VT, WS>(f, sh, bk, k); })
  if (ws) {
    if (iv && sp) EMU_GO(true, 1, true);
    if (iv) EMU_GO(false, 1, true);
    if (sp) EMU_GO(true, 0, true);
    EMU_GO(false, 0, true);
  }
  if (iv && sp) EMU_GO(true, 1, false);
  if (iv) EMU_GO(false, 1, false);
  if (sp) EMU_GO(true, 0, false);
  EMU_GO(false, 0, false);
#undef EMU_GO
}

}  // namespace

extern "C" int emu_parse_ws(const uint8_t *text, uint64_t nbytes, const uint64_t *ccs, int nchunks_in,
                            const dmlc_amd_params *prm, const dmlc_amd_csr *out, uint64_t *chunk_table,
                            uint64_t *res /* 16 */) {
  const uint32_t delim = (uint32_t)prm->delimiter & 0xFFu;
  const int sp_delim = csv_single_pass_delim(delim);
  const bool use_fast = prm->format == DMLC_AMD_CSV && nbytes > 0 && sp_delim != 0 &&
                        csv_single_pass_columns(prm->value_type, prm->label_column, prm->weight_column) &&
                        !(prm->flags & DMLC_AMD_FLAG_EXACT);
  dmlc_amd_params xprm = *prm;
  xprm.flags |= DMLC_AMD_FLAG_EXACT;
  if (!use_fast) return emu_parse(text, nbytes, ccs, nchunks_in, prm->format == DMLC_AMD_CSV ? &xprm : prm, out,
                                  chunk_table, res);
  // FillData ranges as ParseBlock units (emu.cpp emu_parse)
  const int upc = prm->nthread > 1 ? prm->nthread : 1;
  std::vector<uint64_t> unit_starts;
  const uint64_t *cs = ccs;
  int nchunks = nchunks_in;
  if (upc > 1) {
    for (int c = 0; c < nchunks_in; ++c) {
      const uint64_t head = ccs[c], size = ccs[c + 1] - head, nstep = (size + upc - 1) / upc;
      for (int t = 0; t < upc; ++t) {
        const uint64_t sb = (uint64_t)t * nstep < size ? (uint64_t)t * nstep : size;
        uint64_t p = head + sb, r = head;
        for (; p > head; --p)
          if (p < head + size && (text[p] == '\n' || text[p] == '\r')) {
            r = p;
            break;
          }
        unit_starts.push_back(t == 0 ? head : r);
      }
    }
    unit_starts.push_back(nbytes);
    cs = unit_starts.data();
    nchunks = nchunks_in * upc;
  }
  const bool count_only = prm->flags & DMLC_AMD_FLAG_COUNT_ONLY;
  std::memset(res, 0, 16 * 8);
  res[8] = ~0ull;
  if (!count_only) chunk_prefill(chunk_table, nchunks);
  uint32_t gate = 0;
  std::vector<uint64_t> labsum(kLabShards * 8, 0);
  unsigned long long ferr = ~0ull;
  const uint64_t nft = (nbytes + fast::kTile - 1) / fast::kTile;
  std::vector<uint64_t> lb(nft * kCsvLbWords + 1, 0);
  FastCsvArgs f;
  std::memset(&f, 0, sizeof(f));
  f.text = text;
  f.n = nbytes;
  f.cs = cs;
  f.nchunk = nchunks;
  f.ntiles = (uint32_t)nft;
  f.wide = prm->index_bits == 64;
  f.delim = delim;
  f.ws = sp_delim == 2;
  f.label_col = prm->label_column;
  f.weight_col = prm->value_type == DMLC_AMD_F32 ? prm->weight_column : -1;
  f.vtype = prm->value_type;
  f.label = reinterpret_cast<float *>(out->label);
  f.weight = out->weight;
  f.labsum = labsum.data();
  f.offset = out->offset;
  f.index = out->index;
  f.value = out->value;
  for (int i = 0; i < 8; ++i) f.cap[i] = out->cap[i];
  f.chunk_tab = chunk_table;
  f.lb = lb.data();
  f.gate = &gate;
  f.err = &ferr;
  f.res = res;
  for (uint64_t k = 0; k < nft; ++k) {
    fcsv::Shared *sh = new fcsv::Shared;
    std::memset(sh, 0xCD, sizeof(*sh));  // LDS is uninitialised on the GPU
    if (count_only) run_fast_tile<1>(f, *sh, (uint32_t)k);
    else run_fast_tile<2>(f, *sh, (uint32_t)k);
    delete sh;
  }
  if (f.label_col >= 0 || f.weight_col >= 0) {  // label_check_kernel
    uint64_t s0 = 0, s1 = 0, s2 = 0;
    for (int i = 0; i < kLabShards; ++i) {
      s0 += labsum[i * 8];
      s1 += labsum[i * 8 + 1];
      s2 += labsum[i * 8 + 2];
    }
    if (s0 != 0 || s1 != 0 || s2 != 0) gate |= 1u;
  }
  if (gate) return emu_parse(text, nbytes, ccs, nchunks_in, &xprm, out, chunk_table, res);  // prints path=exact
  std::fprintf(stderr, "emu: csv path=fast\n");
  res[8] = ferr;
  if (res[8] == ~0ull) res[8] = 0;
  if (!count_only) chunk_fixup(chunk_table, nchunks, res);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 12) {
    std::fprintf(stderr, "usage: see emu.cpp\n");
    return 2;
  }
  dmlc_amd_params prm;
  std::memset(&prm, 0, sizeof(prm));
  prm.format = std::atoi(argv[1]);
  prm.index_bits = std::atoi(argv[2]);
  prm.value_type = std::atoi(argv[3]);
  prm.indexing_mode = std::atoi(argv[4]);
  prm.label_column = std::atoi(argv[5]);
  prm.weight_column = std::atoi(argv[6]);
  prm.delimiter = std::atoi(argv[7]);
  prm.tile_bytes = (uint32_t)std::atoi(argv[8]);
  if (const char *nt = std::getenv("EMU_NTHREAD")) prm.nthread = std::atoi(nt);
  std::vector<char> text = slurp(argv[9]);
  std::vector<char> craw = slurp(argv[10]);
  std::vector<uint64_t> cs(craw.size() / 8);
  std::memcpy(cs.data(), craw.data(), craw.size());
  const int nch = (int)cs.size() - 1;
  // exact-size heap copy of the text so ASan sees reads past its end
  uint8_t *t = (uint8_t *)std::malloc(text.size() ? text.size() : 1);
  std::memcpy(t, text.data(), text.size());
  uint64_t res[16];
  dmlc_amd_csr csr;
  std::memset(&csr, 0, sizeof(csr));
  const uint32_t xf = std::getenv("EMU_EXACT") ? DMLC_AMD_FLAG_EXACT : 0u;
  prm.flags = DMLC_AMD_FLAG_COUNT_ONLY | xf;
  emu_parse_ws(t, text.size(), cs.data(), nch, &prm, &csr, nullptr, res);
  prm.flags = xf;
  const size_t vsz = prm.value_type == DMLC_AMD_I64 ? 8 : 4, isz = prm.index_bits == 64 ? 8 : 4;
  // exact-size outputs: a store past the counted sizes is an ASan error
  std::vector<uint64_t> offset(res[0] + 1);
  void *label = std::malloc(res[5] * vsz + 1), *value = std::malloc(res[2] * vsz + 1),
       *index = std::malloc(res[1] * isz + 1), *field = std::malloc(res[6] * isz + 1);
  std::vector<float> weight(res[3] + 1);
  std::vector<uint64_t> qid(res[4] + 1);
  const int upc = prm.nthread > 1 && !text.empty() ? prm.nthread : 1;
  std::vector<uint64_t> chunks((nch > 0 ? nch * upc : 1) * 8, 0);
  csr.offset = offset.data();
  csr.label = label;
  csr.weight = weight.data();
  csr.qid = qid.data();
  csr.index = index;
  csr.field = field;
  csr.value = value;
  uint64_t caps[8] = {res[0], res[1], res[2], res[3], res[4], res[5], res[6], 0};
  std::memcpy(csr.cap, caps, sizeof(caps));
  uint64_t res2[16];
  emu_parse_ws(t, text.size(), cs.data(), nch, &prm, &csr, chunks.data(), res2);
  std::string o = argv[11];
  dump(o + ".res", res2, sizeof(res2));
  dump(o + ".offset", offset.data(), offset.size() * 8);
  dump(o + ".label", label, res2[5] * vsz);
  dump(o + ".weight", weight.data(), res2[3] * 4);
  dump(o + ".qid", qid.data(), res2[4] * 8);
  dump(o + ".index", index, res2[1] * isz);
  dump(o + ".field", field, res2[6] * isz);
  dump(o + ".value", value, res2[2] * vsz);
  dump(o + ".chunks", chunks.data(), chunks.size() * 8);
  std::free(t);
  std::free(label);
  std::free(value);
  std::free(index);
  std::free(field);
  return 0;
}
