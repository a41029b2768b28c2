// hda_yaml.cpp -- YAML-subset parser and argument mapping (see hda_yaml.h).
// Own implementation of the grammar documented in SURVEY.md App. B; the key names and the
// string->enum maps are the reference's input contract (src/internal/amg.c:23-90,245-459,
// src/internal/pcg.c:15-25, src/internal/gmres.c:16-27, src/internal/args.c:30-45,
// src/internal/linsys.c:290-320,360-385).
#include "hda_yaml.h"

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <sstream>

namespace hda {

static std::string trim(const std::string &s)
{
   size_t a = 0, b = s.size();
   while (a < b && isspace((unsigned char)s[a])) a++;
   while (b > a && isspace((unsigned char)s[b - 1])) b--;
   return s.substr(a, b - a);
}
static std::string lower(std::string s)
{
   for (auto &c : s) c = (char)tolower((unsigned char)c);
   return s;
}
static std::string unquote(const std::string &s)
{
   if (s.size() >= 2 && ((s.front() == '"' && s.back() == '"') || (s.front() == '\'' && s.back() == '\''))) return s.substr(1, s.size() - 2);
   return s;
}
static bool keeps_case(const std::string &key)
{
   return key.find("filename") != std::string::npos || key.find("dirname") != std::string::npos ||
          key.find("basename") != std::string::npos || key == "name";
}

YNode *YNode::find(const std::string &k)
{
   for (auto &c : kids)
      if (c->key == k) return c.get();
   return nullptr;
}
YNode *YNode::get_or_add(const std::string &k)
{
   if (YNode *n = find(k)) return n;
   kids.emplace_back(new YNode());
   kids.back()->key = k;
   return kids.back().get();
}

static void set_keyval(YNode &n, const std::string &rawkey, const std::string &rawval)
{
   n.key = lower(trim(rawkey));
   std::string v = unquote(trim(rawval));
   n.val         = keeps_case(n.key) ? v : lower(v);
}

// "{a: b, c: d}" -> children of n
static void parse_flow(YNode &n, const std::string &flow)
{
   std::string body = trim(flow);
   if (body.size() >= 2 && body.front() == '{' && body.back() == '}') body = body.substr(1, body.size() - 2);
   size_t pos = 0;
   int    depth = 0;
   std::string cur;
   auto flush = [&]() {
      std::string item = trim(cur);
      cur.clear();
      if (item.empty()) return;
      size_t c = item.find(':');
      n.kids.emplace_back(new YNode());
      if (c == std::string::npos) set_keyval(*n.kids.back(), item, "");
      else
      {
         std::string v = trim(item.substr(c + 1));
         if (!v.empty() && v.front() == '{')
         {
            set_keyval(*n.kids.back(), item.substr(0, c), "");
            parse_flow(*n.kids.back(), v);
         }
         else set_keyval(*n.kids.back(), item.substr(0, c), v);
      }
   };
   for (; pos < body.size(); pos++)
   {
      char ch = body[pos];
      if (ch == '{' || ch == '[') depth++;
      if (ch == '}' || ch == ']') depth--;
      if (ch == ',' && depth == 0) flush();
      else cur.push_back(ch);
   }
   flush();
}

uint32_t yaml_parse(const std::string &text, YNode &root, std::string &message)
{
   struct Frame {
      int    level;
      YNode *node;
   };
   std::vector<Frame> stack{{-1, &root}};
   int                base = 0, lineno = 0;
   size_t             p = 0;
   while (p <= text.size())
   {
      size_t      e = text.find('\n', p);
      std::string line = text.substr(p, e == std::string::npos ? std::string::npos : e - p);
      p = (e == std::string::npos) ? text.size() + 1 : e + 1;
      lineno++;
      if (!line.empty() && line.back() == '\r') line.pop_back();
      size_t hash = line.find('#');
      if (hash != std::string::npos) line = line.substr(0, hash);
      size_t ind = 0;
      while (ind < line.size() && (line[ind] == ' ' || line[ind] == '\t'))
      {
         if (line[ind] == '\t')
         {
            message = "line " + std::to_string(lineno) + ": tab used for indentation";
            return ERR_YAML_MIXED_INDENT;
         }
         ind++;
      }
      std::string content = trim(line);
      if (content.empty()) continue;
      if (ind > 0 && base == 0) base = (int)ind;
      if (base && ind % (size_t)base)
      {
         message = "line " + std::to_string(lineno) + ": indentation is not a multiple of " + std::to_string(base);
         return ERR_YAML_INVALID_INDENT;
      }
      int level = base ? (int)ind / base : 0;
      while (stack.size() > 1 && stack.back().level >= level) stack.pop_back();
      if (level > stack.back().level + 1)
      {
         message = "line " + std::to_string(lineno) + ": indentation jumps more than one level";
         return ERR_YAML_INVALID_INDENT_JUMP;
      }
      YNode *parent = stack.back().node;
      bool   dash   = content[0] == '-' && (content.size() == 1 || content[1] == ' ');
      if (dash)
      {
         parent->kids.emplace_back(new YNode());
         YNode *item    = parent->kids.back().get();
         item->key      = "-";
         item->seq_item = true;
         stack.push_back({level, item});
         content = trim(content.substr(1));
         if (content.empty()) continue;
         if (content.front() == '{') { parse_flow(*item, content); continue; }
         // scalar item: "- file.yml", "- [0, 2]", "- \"quoted: text\"" (a list-valued include, a sequence of
         // flow lists).  A ':' inside brackets or quotes does not make it a mapping.
         {
            bool   mapping = false;
            int    depth   = 0;
            char   quote   = 0;
            for (char ch : content)
            {
               if (quote) { if (ch == quote) quote = 0; continue; }
               if (ch == '"' || ch == '\'') quote = ch;
               else if (ch == '[' || ch == '{') depth++;
               else if (ch == ']' || ch == '}') depth--;
               else if (ch == ':' && depth == 0) { mapping = true; break; }
            }
            if (!mapping)
            {
               item->val = unquote(content); // case kept: it may be a file name
               continue;
            }
         }
         parent = item;
         level  = level + 1;
      }
      size_t c = content.find(':');
      if (c == std::string::npos)
      {
         message = "line " + std::to_string(lineno) + ": expected 'key: value'";
         return ERR_YAML_INVALID_DIVISOR;
      }
      parent->kids.emplace_back(new YNode());
      YNode      *n = parent->kids.back().get();
      std::string v = trim(content.substr(c + 1));
      if (!v.empty() && v.front() == '{')
      {
         set_keyval(*n, content.substr(0, c), "");
         parse_flow(*n, v);
      }
      else set_keyval(*n, content.substr(0, c), v);
      stack.push_back({level, n});
   }
   return ERR_NONE;
}

static void print_node(const YNode &n, int indent, FILE *out);
static void print_kv(const YNode &n, int indent, const char *prefix, FILE *out)
{
   fprintf(out, "%*s%s%s: %s\n", indent, "", prefix, n.key.c_str(), n.val.c_str());
   for (auto &k : n.kids) print_node(*k, indent + 2 + (int)strlen(prefix), out);
}
static void print_node(const YNode &n, int indent, FILE *out)
{
   if (n.seq_item)
   {
      if (n.kids.empty() && !n.val.empty()) { fprintf(out, "%*s- %s\n", indent, "", n.val.c_str()); return; }
      bool first = true;
      for (auto &k : n.kids)
      {
         print_kv(*k, indent, first ? "- " : "  ", out);
         first = false;
      }
      return;
   }
   print_kv(n, indent, "", out);
}
void yaml_print(const YNode &root, FILE *out)
{
   for (auto &k : root.kids) print_node(*k, 0, out);
}

void yaml_override(YNode &root, const std::string &path, const std::string &value)
{
   std::string p = path;
   while (!p.empty() && p[0] == '-') p.erase(0, 1);
   std::vector<std::string> parts;
   size_t                   pos = 0;
   while (pos <= p.size())
   {
      size_t c = p.find(':', pos);
      parts.push_back(lower(p.substr(pos, c == std::string::npos ? std::string::npos : c - pos)));
      if (c == std::string::npos) break;
      pos = c + 1;
   }
   YNode *cur = &root;
   for (const std::string &part : parts)
   {
      YNode *next = cur->find(part);
      if (!next)
      {
         if (cur != &root && cur->kids.empty() && !cur->val.empty())
         { // value form ("solver: pcg") becomes container form ("solver: {pcg: {...}}")
            const std::string old = cur->val;
            cur->val.clear();
            YNode *mid = cur->get_or_add(old);
            next       = (old == part) ? mid : mid->get_or_add(part);
         }
         else next = cur->get_or_add(part);
      }
      cur = next;
   }
   std::string v = unquote(trim(value));
   cur->val      = keeps_case(cur->key) ? v : lower(v);
}

// --------------------------------------------------------------- value maps

typedef std::map<std::string, int> StrMap;
static const StrMap kOnOff = {{"on", 1}, {"yes", 1}, {"true", 1}, {"1", 1}, {"off", 0}, {"no", 0}, {"false", 0}, {"0", 0}};
static const StrMap kInterp = {{"mod_classical", 0}, {"least_squares", 1}, {"mod_classical_he", 2}, {"direct_sep_weights", 3},
                               {"multipass", 4}, {"multipass_sep_weights", 5}, {"extended+i", 6}, {"extended+i_c", 7},
                               {"standard", 8}, {"standard_sep_weights", 9}, {"blk_classical", 10}, {"blk_classical_diag", 11},
                               {"f_f", 12}, {"f_f1", 13}, {"extended", 14}, {"mm_extended", 16}, {"mm_extended+i", 17},
                               {"mm-ext+i", 17}, {"mm_extended+e", 18}, {"mm-ext+e", 18}, {"blk_direct", 24}, {"one_point", 100}};
static const StrMap kPoints = {{"all", 0}, {"air", 1}}; // relaxation.points (reference src/internal/amg.c:400-408)
static const StrMap kRestrict = {{"p_transpose", 0}, {"air_1", 1}, {"air_2", 2}, {"neumann_air_0", 3}, {"neumann_air_1", 4},
                                 {"neumann_air_2", 5}, {"air_1.5", 15}};
static const StrMap kCoarsen = {{"cljp", 0}, {"rs", 1}, {"rs3", 3}, {"falgout", 6}, {"pmis", 8}, {"hmis", 10}};
static const StrMap kAggInterp = {{"2_stage_extended+i", 1}, {"2_stage_standard", 2}, {"2_stage_extended", 3}, {"multipass", 4},
                                  {"mm_extended", 5}, {"mm_extended+i", 6}, {"mm_extended+e", 7}};
static const StrMap kRelax = {{"jacobi_non_mv", 0}, {"forward-hgs", 3}, {"backward-hgs", 4}, {"chaotic-hgs", 5}, {"hsgs", 6},
                              {"jacobi", 7}, {"l1-hsgs", 8}, {"ge", 9}, {"forward-solve", 10}, {"2gs-it1", 11}, {"2gs-it2", 12},
                              {"forward-hl1gs", 13}, {"backward-hl1gs", 14}, {"cg", 15}, {"chebyshev", 16}, {"l1-jacobi", 18},
                              {"l1sym-hgs", 89}, {"lu_piv", 99}, {"lu_inv", 199}};
static const StrMap kSmoothType = {{"fsai", 4}, {"ilu", 5}, {"schwarz", 6}, {"pilut", 7}, {"parasails", 8}, {"euclid", 9}};
static const StrMap kRhsMode = {{"zeros", 0}, {"ones", 1}, {"file", 2}, {"random", 3}, {"randsol", 4}};
static const StrMap kX0Mode = {{"zeros", 0}, {"ones", 1}, {"file", 2}, {"random", 3}, {"previous", 4}};
static const StrMap kLsType = {{"online", 0}, {"ij", 1}, {"parcsr", 2}, {"mtx", 3}};
static const StrMap kExec = {{"host", 0}, {"device", 1}};

struct Ctx {
   uint32_t    err = 0;
   std::string msg;
   void fail(uint32_t e, const std::string &m)
   {
      if (!err) msg = m;
      err |= e;
   }
};

static int to_int(Ctx &c, const YNode &n, const StrMap *map)
{
   if (map)
   {
      auto it = map->find(n.val);
      if (it != map->end()) return it->second;
   }
   char *end = nullptr;
   long  v   = strtol(n.val.c_str(), &end, 10);
   if (n.val.empty() || (end && *end)) c.fail(ERR_INVALID_VAL, "invalid value '" + n.val + "' for key '" + n.key + "'");
   return (int)v;
}
static double to_double(Ctx &c, const YNode &n)
{
   char  *end = nullptr;
   double v   = strtod(n.val.c_str(), &end);
   if (n.val.empty() || (end && *end)) c.fail(ERR_INVALID_VAL, "invalid value '" + n.val + "' for key '" + n.key + "'");
   return v;
}

struct Field {
   const char   *name;
   int          *i;
   double       *d;
   const StrMap *map;
};
static void apply_fields(Ctx &c, YNode &sec, const std::vector<Field> &f, const std::vector<std::string> &ignored = {})
{
   for (auto &k : sec.kids)
   {
      bool hit = false;
      for (auto &fl : f)
         if (k->key == fl.name)
         {
            if (fl.i) *fl.i = to_int(c, *k, fl.map);
            else *fl.d = to_double(c, *k);
            hit = true;
            break;
         }
      if (!hit && std::find(ignored.begin(), ignored.end(), k->key) == ignored.end())
         c.fail(ERR_INVALID_KEY, "unknown key '" + k->key + "' under '" + sec.key + "'");
   }
}

static uint32_t expand_includes_rec(YNode &node, const std::string &base_dir, std::vector<std::string> &stack, std::string &message)
{
   for (size_t i = 0; i < node.kids.size(); i++)
   {
      YNode &k = *node.kids[i];
      if (k.key == "include" && k.kids.empty() && !k.val.empty())
      {
         std::string path = k.val;
         if (path[0] != '/' && !base_dir.empty()) path = base_dir + "/" + path;
         if (stack.size() >= 10) { message = "YAML include depth exceeded max depth 10"; return ERR_YAML_TREE_INVALID; }
         if (std::find(stack.begin(), stack.end(), path) != stack.end()) { message = "YAML include cycle detected at '" + path + "'"; return ERR_YAML_TREE_INVALID; }
         FILE *f = fopen(path.c_str(), "r");
         if (!f) { message = "cannot open included YAML file '" + path + "'"; return ERR_FILE_NOT_FOUND; }
         std::string text;
         char        buf[4096];
         size_t      n;
         while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
         fclose(f);
         YNode    sub;
         uint32_t e = yaml_parse(text, sub, message);
         if (e) return e;
         stack.push_back(path);
         const size_t slash = path.find_last_of('/');
         e                  = expand_includes_rec(sub, slash == std::string::npos ? std::string() : path.substr(0, slash), stack, message);
         stack.pop_back();
         if (e) return e;
         // splice the included top-level entries where the include stood
         std::vector<std::unique_ptr<YNode>> tail;
         for (size_t j = i + 1; j < node.kids.size(); j++) tail.push_back(std::move(node.kids[j]));
         node.kids.resize(i);
         for (auto &q : sub.kids) node.kids.push_back(std::move(q));
         const size_t added = node.kids.size() - i;
         for (auto &q : tail) node.kids.push_back(std::move(q));
         i += added;
         i--;
         continue;
      }
      if (k.key == "include" && k.val.empty() && !k.kids.empty())
      { // list-valued include (reference src/internal/yaml.c:1863-2003): the top-level entries of every listed file become ONE
        // sequence item appended to this node -- "amg: include: [a.yml, b.yml]" makes two preconditioner variants
         std::vector<std::string> paths;
         for (auto &q : k.kids)
            if (q->seq_item && q->kids.empty() && !q->val.empty()) paths.push_back(q->val);
            else { message = "include: expected a list of file names"; return ERR_YAML_TREE_INVALID; }
         node.kids.erase(node.kids.begin() + (long)i);
         for (const std::string &rel : paths)
         {
            std::string path = rel;
            if (path[0] != '/' && !base_dir.empty()) path = base_dir + "/" + path;
            if (stack.size() >= 10) { message = "YAML include depth exceeded max depth 10"; return ERR_YAML_TREE_INVALID; }
            if (std::find(stack.begin(), stack.end(), path) != stack.end()) { message = "YAML include cycle detected at '" + path + "'"; return ERR_YAML_TREE_INVALID; }
            FILE *f = fopen(path.c_str(), "r");
            if (!f) { message = "cannot open included YAML file '" + path + "'"; return ERR_FILE_NOT_FOUND; }
            std::string text;
            char        buf[4096];
            size_t      n;
            while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
            fclose(f);
            YNode    sub;
            uint32_t e = yaml_parse(text, sub, message);
            if (e) return e;
            stack.push_back(path);
            const size_t slash = path.find_last_of('/');
            e                  = expand_includes_rec(sub, slash == std::string::npos ? std::string() : path.substr(0, slash), stack, message);
            stack.pop_back();
            if (e) return e;
            node.kids.emplace_back(new YNode());
            YNode *item    = node.kids.back().get();
            item->key      = "-";
            item->seq_item = true;
            for (auto &q : sub.kids) item->kids.push_back(std::move(q));
         }
         i--; // the include node is gone: look at what now stands at its place
         continue;
      }
      uint32_t e = expand_includes_rec(k, base_dir, stack, message);
      if (e) return e;
   }
   return 0;
}
uint32_t yaml_expand_includes(YNode &root, const std::string &base_dir, std::string &message)
{
   std::vector<std::string> stack;
   return expand_includes_rec(root, base_dir, stack, message);
}

void KrylovArgs::defaults_for(int m)
{
   *this  = KrylovArgs();
   method = m;
   if (m == 1 || m == 2) max_iter = 300;
   if (m == 3) max_iter = 100;
}

// ILU_FIELDS and the type names of hypredrv_ILUGetValidValues (reference src/internal/ilu.c:15-28, :45-55)
static const StrMap kIluType = {{"bj-iluk", 0}, {"bj-ilut", 1}, {"gmres-iluk", 10}, {"gmres-ilut", 11}, {"nsh-iluk", 20}, {"nsh-ilut", 21},
                                {"ras-iluk", 30}, {"ras-ilut", 31}, {"ddpq-gmres-iluk", 40}, {"ddpq-gmres-ilut", 41}, {"rap-mod-ilu0", 50}};
static void ilu_fields(Ctx &c, YNode &sec, IluArgs &a)
{
   apply_fields(c, sec,
                {{"max_iter", &a.max_iter, nullptr, nullptr}, {"print_level", &a.print_level, nullptr, nullptr}, {"type", &a.type, nullptr, &kIluType},
                 {"fill_level", &a.fill_level, nullptr, nullptr}, {"reordering", &a.reordering, nullptr, nullptr},
                 {"tri_solve", &a.tri_solve, nullptr, &kOnOff}, {"lower_jac_iters", &a.lower_jac_iters, nullptr, nullptr},
                 {"upper_jac_iters", &a.upper_jac_iters, nullptr, nullptr}, {"max_row_nnz", &a.max_row_nnz, nullptr, nullptr},
                 {"schur_max_iter", &a.schur_max_iter, nullptr, nullptr}, {"droptol", nullptr, &a.droptol, nullptr},
                 {"nsh_droptol", nullptr, &a.nsh_droptol, nullptr}, {"tolerance", nullptr, &a.tolerance, nullptr}});
}

// Schwarz_FIELDS and the name maps of hypredrv_SchwarzGetValidValues (reference src/internal/schwarz.c:20-34, :48-66).  Every name
// parses; what is not built is refused at HYPREDRV_PreconCreate.
static const StrMap kSchwarzVariant = {{"mp", 0}, {"ad", 1}, {"par-ad", 2}, {"par-mp", 3}, {"mp-fw", 4}, {"ras-iluk", 10}, {"as-iluk", 11},
                                       {"ras-ilut", 20}, {"as-ilut", 21}, {"ras-amg", 30}, {"as-amg", 31}, {"ras-spdirect", 40}, {"as-spdirect", 41}};
static const StrMap kSchwarzLocal = {{"iluk", 0}, {"ilut", 1}, {"amg", 2}, {"spdirect", 3}, {"superlu", 3}};
static void schwarz_fields(Ctx &c, YNode &sec, SchwarzArgs &a)
{
   apply_fields(c, sec,
                {{"variant", &a.variant, nullptr, &kSchwarzVariant}, {"overlap", &a.overlap, nullptr, nullptr},
                 {"domain_type", &a.domain_type, nullptr, nullptr}, {"num_functions", &a.num_functions, nullptr, nullptr},
                 {"use_nonsymm", &a.use_nonsymm, nullptr, &kOnOff}, {"local_solver_type", &a.local_solver_type, nullptr, &kSchwarzLocal},
                 {"iluk_level_of_fill", &a.iluk_level_of_fill, nullptr, nullptr}, {"ilut_max_nnz_row", &a.ilut_max_nnz_row, nullptr, nullptr},
                 {"max_iter", &a.max_iter, nullptr, nullptr}, {"print_level", &a.print_level, nullptr, nullptr},
                 {"logging", &a.logging, nullptr, nullptr}, {"relax_weight", nullptr, &a.relax_weight, nullptr},
                 {"ilut_droptol", nullptr, &a.ilut_droptol, nullptr}, {"tolerance", nullptr, &a.tolerance, nullptr}});
}

// FSAI_FIELDS and the algo_type names of hypredrv_FSAIGetValidValues (reference src/internal/fsai.c:15-27, :45).  Every value parses;
// what is not built (the adaptive algorithms, a tolerance, numbers out of range) is refused at HYPREDRV_PreconCreate / at setup.
static const StrMap kFsaiAlgo = {{"bj-afsai", 1}, {"bj-afsai-omp", 2}, {"bj-sfsai", 3}};
static void fsai_fields(Ctx &c, YNode &sec, FsaiArgs &a)
{
   apply_fields(c, sec,
                {{"max_iter", &a.max_iter, nullptr, nullptr}, {"print_level", &a.print_level, nullptr, nullptr},
                 {"algo_type", &a.algo_type, nullptr, &kFsaiAlgo}, {"ls_type", &a.ls_type, nullptr, nullptr},
                 {"max_steps", &a.max_steps, nullptr, nullptr}, {"max_step_size", &a.max_step_size, nullptr, nullptr},
                 {"max_nnz_row", &a.max_nnz_row, nullptr, nullptr}, {"num_levels", &a.num_levels, nullptr, nullptr},
                 {"eig_max_iters", &a.eig_max_iters, nullptr, nullptr}, {"threshold", nullptr, &a.threshold, nullptr},
                 {"kap_tolerance", nullptr, &a.kap_tolerance, nullptr}, {"tolerance", nullptr, &a.tolerance, nullptr}});
}

// AMS_FIELDS (reference src/internal/ams.c:37-63): 24 keys, numbers only (keys arrive in lower case: alpha_Pmax is alpha_pmax
// here).  Every value parses; what is not built is refused at HYPREDRV_PreconCreate.
static void ams_fields(Ctx &c, YNode &sec, AmsArgs &a)
{
   apply_fields(c, sec,
                {{"dimension", &a.dimension, nullptr, nullptr}, {"max_iter", &a.max_iter, nullptr, nullptr}, {"print_level", &a.print_level, nullptr, nullptr},
                 {"cycle_type", &a.cycle_type, nullptr, nullptr}, {"tolerance", nullptr, &a.tolerance, nullptr},
                 {"relax_type", &a.relax_type, nullptr, nullptr}, {"relax_times", &a.relax_times, nullptr, nullptr},
                 {"relax_weight", nullptr, &a.relax_weight, nullptr}, {"omega", nullptr, &a.omega, nullptr}, {"proj_freq", &a.proj_freq, nullptr, nullptr},
                 {"alpha_coarsen_type", &a.alpha_coarsen_type, nullptr, nullptr}, {"alpha_agg_levels", &a.alpha_agg_levels, nullptr, nullptr},
                 {"alpha_relax_type", &a.alpha_relax_type, nullptr, nullptr}, {"alpha_strength_threshold", nullptr, &a.alpha_strength_threshold, nullptr},
                 {"alpha_interp_type", &a.alpha_interp_type, nullptr, nullptr}, {"alpha_pmax", &a.alpha_Pmax, nullptr, nullptr},
                 {"alpha_coarse_relax_type", &a.alpha_coarse_relax_type, nullptr, nullptr},
                 {"beta_coarsen_type", &a.beta_coarsen_type, nullptr, nullptr}, {"beta_agg_levels", &a.beta_agg_levels, nullptr, nullptr},
                 {"beta_relax_type", &a.beta_relax_type, nullptr, nullptr}, {"beta_strength_threshold", nullptr, &a.beta_strength_threshold, nullptr},
                 {"beta_interp_type", &a.beta_interp_type, nullptr, nullptr}, {"beta_pmax", &a.beta_Pmax, nullptr, nullptr},
                 {"beta_coarse_relax_type", &a.beta_coarse_relax_type, nullptr, nullptr}});
}

// mgr block (reference src/internal/mgr.c:1736-1870; value maps :1553-1721)
static const StrMap kMgrInterp = {{"injection", 0}, {"l1-jacobi", 1}, {"jacobi", 2}, {"classical-mod", 3}, {"approx-inv", 4}, {"blk-jacobi", 12},
                                  {"blk-rowlump", 13}, {"blk-rowsum", 13}, {"blk-absrowsum", 14}};
static const StrMap kMgrRestrict = {{"injection", 0}, {"jacobi", 2}, {"approx-inv", 3}, {"air_1", 4}, {"air_1.5", 5}, {"blk-jacobi", 12},
                                    {"cpr-like", 13}, {"columped", 14}, {"columped-partial", 15}};
static const StrMap kMgrCoarse = {{"rap", 0}, {"galerkin", 0}, {"non-galerkin", 1}, {"cpr-like-diag", 2}, {"cpr-like-bdiag", 3}, {"approx-inv", 4}, {"acc", 5}};
static const StrMap kMgrFrelax = {{"", -1}, {"none", -1}, {"single", 7}, {"jacobi", 7}, {"l1-jacobi", 18}, {"v(1,0)", 1}, {"amg", 2}, {"mgr", 100},
                                  {"chebyshev", 16}, {"ilu", 32}, {"ge", 9}, {"spdirect", 29}, {"ge-piv", 99}, {"ge-inv", 199}, {"fsai", 33}, {"schwarz", 34}};
static const StrMap kMgrGrelax = {{"", -1}, {"none", -1}, {"blk-jacobi", 0}, {"blk-gs", 1}, {"mixed-gs", 2}, {"amg", 20}, {"h-fgs", 3}, {"h-bgs", 4},
                                  {"ch-gs", 5}, {"h-ssor", 6}, {"euclid", 8}, {"2stg-fgs", 11}, {"2stg-bgs", 12}, {"l1-hfgs", 13}, {"l1-hbgs", 14},
                                  {"ilu", 16}, {"spdirect", 29}, {"l1-hsgs", 88}, {"fsai", 33}, {"schwarz", 34}};
static const StrMap kMgrCoarsest = {{"def", -1}, {"amg", 0}, {"spdirect", 29}, {"ilu", 32}, {"fsai", 33}, {"schwarz", 34}};
static const StrMap kMgrCycle = {{"v", 1}, {"w", 2}, {"1", 1}, {"2", 2}};

static void amg_fields(Ctx &c, YNode &sec, AmgArgs &a);

static std::vector<int> int_list(Ctx &c, YNode &k, const char *what)
{
   std::string s = k.val;
   for (auto &q : k.kids) s += " " + (q->val.empty() ? q->key : q->val); // block sequence form
   for (char &ch : s)
      if (ch == '[' || ch == ']' || ch == ',') ch = ' ';
   std::istringstream is(s);
   std::string        tok;
   std::vector<int>   out;
   while (is >> tok)
   {
      char *end = nullptr;
      long  v   = strtol(tok.c_str(), &end, 10);
      if (!end || *end) { c.fail(ERR_INVALID_VAL, std::string(what) + ": '" + tok + "' is not an integer label (symbolic dof labels are not supported)"); break; }
      out.push_back((int)v);
   }
   return out;
}

// nested Krylov components (reference src/internal/mgr.c:683-700 MGRIsNestedKrylovKey: any solver type name)
static bool is_krylov_name(const std::string &k) { return k == "pcg" || k == "gmres" || k == "fgmres" || k == "bicgstab"; }

static void ilu_fields(Ctx &c, YNode &sec, IluArgs &a);
static void krylov_fields(Ctx &c, YNode &sec, KrylovArgs &k);
static int  solver_method(const std::string &name);
// A nested Krylov block (reference hypredrv_NestedKrylovSetArgsFromYAML, src/internal/krylov.c:360-414): the node's key names the
// method, `preconditioner:` is detached and parsed on its own, the rest are the method's solver keys.
static void nested_krylov(Ctx &c, YNode &node, NestedKrylovArgs &nk, const std::string &where)
{
   nk.set = true;
   nk.solver.defaults_for(solver_method(node.key));
   std::unique_ptr<YNode> pre;
   for (size_t i = 0; i < node.kids.size(); i++)
      if (node.kids[i]->key == "preconditioner")
      {
         pre = std::move(node.kids[i]);
         node.kids.erase(node.kids.begin() + (long)i);
         break;
      }
   krylov_fields(c, node, nk.solver);
   if (!pre) return;
   auto named = [&](const std::string &name, YNode *block) {
      if (name == "amg") { nk.precon = 0; if (block) amg_fields(c, *block, nk.amg); }
      else if (name == "ilu") { nk.precon = 2; if (block) ilu_fields(c, *block, nk.ilu); }
      else if (name == "none") nk.precon = 99;
      else if (name == "mgr" || name == "fsai" || name == "schwarz")
         c.fail(ERR_INVALID_VAL, "mgr: '" + name + "' as preconditioner of the nested " + node.key + " of " + where + " is not implemented on MI355X");
      else c.fail(ERR_INVALID_VAL, "unknown nested preconditioner type: '" + name + "'");
   };
   if (pre->kids.empty()) named(pre->val, nullptr);
   else
      for (auto &q : pre->kids) named(q->key, q.get());
   node.kids.push_back(std::move(pre)); // the tree is printed back by print_config_params
}

// f_relaxation / g_relaxation: a flat name, or a block with type / num_sweeps / a nested solver
static void mgr_relax(Ctx &c, YNode &k, const StrMap &map, int &type, int &sweeps, std::string &block, AmgArgs *amg = nullptr,
                      IluArgs *ilu = nullptr, bool *ilu_block = nullptr, NestedKrylovArgs *krylov = nullptr)
{
   if (k.kids.empty())
   {
      type = to_int(c, k, &map);
      return;
   }
   for (auto &q : k.kids)
   {
      if (q->key == "type") type = to_int(c, *q, &map);
      else if (q->key == "num_sweeps") sweeps = to_int(c, *q, nullptr);
      else if (q->key == "amg" && amg)
      {
         auto it = map.find("amg");
         if (it != map.end()) type = it->second;
         amg_fields(c, *q, *amg);
      }
      else if (q->key == "ilu" && ilu)
      {
         auto it = map.find("ilu");
         if (it != map.end()) type = it->second;
         ilu_fields(c, *q, *ilu);
         if (ilu_block) *ilu_block = true;
      }
      else if (q->key == "reuse") { /* component reuse policy: every setup rebuilds here */ }
      else if (q->key == "amg" || q->key == "ilu" || q->key == "fsai" || q->key == "mgr" || q->key == "schwarz")
      {
         block = q->key;
         auto it = map.find(q->key);
         if (it != map.end()) type = it->second;
      }
      else if (is_krylov_name(q->key) && krylov) nested_krylov(c, *q, *krylov, k.key);
      else if (is_krylov_name(q->key))
         c.fail(ERR_INVALID_VAL, "mgr: a nested Krylov solver ('" + q->key + "') as " + k.key + " is not implemented on MI355X");
      else c.fail(ERR_INVALID_KEY, "unknown key '" + q->key + "' under '" + k.key + "'");
   }
}

static void mgr_fields(Ctx &c, YNode &sec, MgrArgs &m)
{
   for (auto &k : sec.kids)
   {
      if (k->key == "level")
      {
         for (auto &lvn : k->kids)
         {
            char *end = nullptr;
            long  id  = strtol(lvn->key.c_str(), &end, 10);
            if (!end || *end || id < 0 || id > 30) { c.fail(ERR_INVALID_KEY, "mgr.level: '" + lvn->key + "' is not a level index (e.g. \"0: { f_dofs: [2] }\")"); continue; }
            if ((size_t)id >= m.level.size()) m.level.resize((size_t)id + 1);
            MgrLevelArgs &L = m.level[(size_t)id];
            for (auto &q : lvn->kids)
            {
               if (q->key == "f_dofs") L.f_dofs = int_list(c, *q, "f_dofs");
               else if (q->key == "prolongation_type") L.prolongation_type = to_int(c, *q, &kMgrInterp);
               else if (q->key == "restriction_type") L.restriction_type = to_int(c, *q, &kMgrRestrict);
               else if (q->key == "coarse_level_type") L.coarse_level_type = to_int(c, *q, &kMgrCoarse);
               else if (q->key == "f_relaxation") mgr_relax(c, *q, kMgrFrelax, L.f_type, L.f_sweeps, L.f_block, &L.f_amg, &L.f_ilu, nullptr, &L.f_krylov);
               else if (q->key == "g_relaxation") mgr_relax(c, *q, kMgrGrelax, L.g_type, L.g_sweeps, L.g_block, nullptr, &L.g_ilu, &L.g_ilu_block);
               else c.fail(ERR_INVALID_KEY, "unknown key '" + q->key + "' under 'mgr.level." + lvn->key + "'");
            }
         }
      }
      else if (k->key == "coarsest_level")
      {
         if (k->kids.empty()) m.coarsest_type = to_int(c, *k, &kMgrCoarsest);
         else
            for (auto &q : k->kids)
            {
               if (q->key == "type") m.coarsest_type = to_int(c, *q, &kMgrCoarsest);
               else if (q->key == "amg") { m.coarsest_type = 0; amg_fields(c, *q, m.coarsest_amg); }
               else if (q->key == "ilu") { m.coarsest_type = 32; ilu_fields(c, *q, m.coarsest_ilu); }
               else if (q->key == "reuse") { /* component reuse policy: every setup rebuilds here */ }
               else if (q->key == "fsai" || q->key == "schwarz" || q->key == "spdirect" || q->key == "krylov")
               {
                  m.coarsest_block = q->key;
                  auto it = kMgrCoarsest.find(q->key);
                  if (it != kMgrCoarsest.end()) m.coarsest_type = it->second;
               }
               else if (is_krylov_name(q->key)) nested_krylov(c, *q, m.coarsest_krylov, "coarsest_level");
               else c.fail(ERR_INVALID_KEY, "unknown key '" + q->key + "' under 'mgr.coarsest_level'");
            }
      }
      else if (k->key == "non_c_to_f") m.non_c_to_f = to_int(c, *k, nullptr);
      else if (k->key == "pmax") m.pmax = to_int(c, *k, nullptr);
      else if (k->key == "max_iter") m.max_iter = to_int(c, *k, nullptr);
      else if (k->key == "num_levels") m.num_levels = to_int(c, *k, nullptr);
      else if (k->key == "relax_type") m.relax_type = to_int(c, *k, &kRelax);
      else if (k->key == "print_level") m.print_level = to_int(c, *k, nullptr);
      else if (k->key == "nonglk_max_elmts") m.nonglk_max_elmts = to_int(c, *k, nullptr);
      else if (k->key == "tolerance") m.tolerance = to_double(c, *k);
      else if (k->key == "coarse_th") m.coarse_th = to_double(c, *k);
      else if (k->key == "cycle")
      {
         // MGRCycleSet (reference src/internal/mgr.c:614-675): 1 | 2 | v | w | v(1,0) | v(0,1) | v(1,1) | w(1,0) | w(0,1) | w(1,1)
         static const std::map<std::string, std::pair<int, int>> names = {
            {"v", {1, 1}}, {"v(1,0)", {1, 1}}, {"v(0,1)", {1, 2}}, {"v(1,1)", {1, 3}}, {"w", {2, 1}}, {"w(1,0)", {2, 1}},
            {"w(0,1)", {2, 2}}, {"w(1,1)", {2, 3}}, {"1", {1, 1}}, {"2", {2, 1}}};
         std::string v = k->val;
         v.erase(std::remove_if(v.begin(), v.end(), [](char ch) { return isspace((unsigned char)ch); }), v.end());
         auto it = names.find(v);
         if (!k->kids.empty() || it == names.end())
            c.fail(ERR_INVALID_VAL, "Invalid MGR cycle '" + k->val + "' (expected 1, 2, v, w, v(1,0), v(0,1), v(1,1), w(1,0), w(0,1), or w(1,1))");
         else
         {
            m.cycle            = it->second.first;
            m.cycle_smooth_pos = it->second.second;
         }
      }
      else c.fail(ERR_INVALID_KEY, "unknown key '" + k->key + "' under 'mgr'");
   }
}

static void krylov_fields(Ctx &c, YNode &sec, KrylovArgs &k)
{
   apply_fields(c, sec,
                {{"max_iter", &k.max_iter, nullptr, nullptr}, {"two_norm", &k.two_norm, nullptr, &kOnOff},
                 {"stop_crit", &k.stop_crit, nullptr, &kOnOff}, {"rel_change", &k.rel_change, nullptr, &kOnOff},
                 {"print_level", &k.print_level, nullptr, nullptr}, {"recompute_res", &k.recompute_res, nullptr, nullptr},
                 {"relative_tol", nullptr, &k.relative_tol, nullptr}, {"absolute_tol", nullptr, &k.absolute_tol, nullptr},
                 {"residual_tol", nullptr, &k.residual_tol, nullptr}, {"conv_fac_tol", nullptr, &k.conv_fac_tol, nullptr},
                 {"min_iter", &k.min_iter, nullptr, nullptr}, {"skip_real_res_check", &k.skip_real_res_check, nullptr, &kOnOff},
                 {"krylov_dim", &k.krylov_dim, nullptr, nullptr}, {"logging", &k.logging, nullptr, nullptr}});
}

static int solver_method(const std::string &name)
{
   if (name == "pcg") return 0;
   if (name == "gmres") return 1;
   if (name == "fgmres") return 2;
   if (name == "bicgstab") return 3;
   return -1;
}

static void parse_solver(Ctx &c, YNode &node, KrylovArgs &k)
{
   if (!node.val.empty() && node.kids.empty())
   { // value-only form: defaults, print_level forced to 0 (reference args.c:379-396)
      int m = solver_method(node.val);
      if (m < 0) return c.fail(ERR_INVALID_VAL, "unknown solver '" + node.val + "'");
      k.defaults_for(m);
      k.print_level = 0;
      return;
   }
   bool        seen = false;
   ScalingArgs sc;
   for (auto &ch : node.kids)
   {
      if (ch->key == "scaling")
      { // solver.scaling (reference src/internal/scaling.c:27-76, detached from the solver block in src/internal/args.c:314-410)
         static const StrMap kScalingType = {{"rhs_l2", 0}, {"dofmap_mag", 1}, {"dofmap_custom", 2}, {"dofmap_row_custom", 3},
                                             {"dofmap_col_custom", 4}, {"dofmap_similarity_custom", 5}};
         for (auto &q : ch->kids)
         {
            if (q->key == "enabled") sc.enabled = to_int(c, *q, &kOnOff);
            else if (q->key == "type") sc.type = to_int(c, *q, &kScalingType);
            else if (q->key == "custom_values")
            {
               std::string t = q->val;
               for (auto &e : q->kids) t += " " + (e->val.empty() ? e->key : e->val);
               for (char &x : t)
                  if (x == '[' || x == ']' || x == ',') x = ' ';
               std::istringstream is(t);
               std::string        tok;
               while (is >> tok)
               {
                  char  *end = nullptr;
                  double v   = strtod(tok.c_str(), &end);
                  if (!end || *end) { c.fail(ERR_INVALID_VAL, "scaling.custom_values: '" + tok + "' is not a number"); break; }
                  sc.custom_values.push_back(v);
               }
            }
            else c.fail(ERR_INVALID_KEY, "unknown key 'scaling." + q->key + "'");
         }
         // dofmap_mag is hypre's HYPRE_ParCSRMatrixComputeScalingTagged: not part of the reference sources, so there
         // is nothing to restate it from -- refuse instead of guessing
         if (sc.enabled && sc.type == 1) c.fail(ERR_INVALID_VAL, "solver.scaling.type dofmap_mag is not implemented on MI355X");
         continue;
      }
      int m = solver_method(ch->key);
      if (m < 0) { c.fail(ERR_INVALID_KEY, "unknown solver '" + ch->key + "'"); continue; }
      k.defaults_for(m);
      krylov_fields(c, *ch, k);
      seen = true;
   }
   if (!seen) c.fail(ERR_MISSING_SOLVER, "solver section names no solver");
   k.scaling = sc;
}

static void amg_fields(Ctx &c, YNode &sec, AmgArgs &a)
{
   for (auto &k : sec.kids)
   {
      if (k->key == "max_iter") a.max_iter = to_int(c, *k, nullptr);
      else if (k->key == "print_level") a.print_level = to_int(c, *k, nullptr);
      else if (k->key == "tolerance") a.tolerance = to_double(c, *k);
      else if (k->key == "interpolation")
         apply_fields(c, *k, {{"prolongation_type", &a.prolongation_type, nullptr, &kInterp},
                              {"restriction_type", &a.restriction_type, nullptr, &kRestrict},
                              {"max_nnz_row", &a.max_nnz_row, nullptr, nullptr}, {"trunc_factor", nullptr, &a.trunc_factor, nullptr},
                              {"restrict_strong_th", nullptr, &a.restrict_strong_th, nullptr},
                              {"restrict_filter_th", nullptr, &a.restrict_filter_th, nullptr}});
      else if (k->key == "coarsening")
         apply_fields(c, *k, {{"type", &a.type, nullptr, &kCoarsen}, {"rap2", &a.rap2, nullptr, &kOnOff},
                              {"mod_rap2", &a.mod_rap2, nullptr, &kOnOff}, {"keep_transpose", &a.keep_transpose, nullptr, &kOnOff},
                              {"sabs", &a.sabs, nullptr, &kOnOff}, {"num_functions", &a.num_functions, nullptr, nullptr},
                              {"filter_functions", &a.filter_functions, nullptr, &kOnOff}, {"nodal", &a.nodal, nullptr, &kOnOff},
                              {"seq_amg_th", &a.seq_amg_th, nullptr, nullptr}, {"min_coarse_size", &a.min_coarse_size, nullptr, nullptr},
                              {"max_coarse_size", &a.max_coarse_size, nullptr, nullptr}, {"max_levels", &a.max_levels, nullptr, nullptr},
                              {"max_row_sum", nullptr, &a.max_row_sum, nullptr}, {"strong_th", nullptr, &a.strong_th, nullptr}});
      else if (k->key == "aggressive")
         apply_fields(c, *k, {{"num_levels", &a.agg_num_levels, nullptr, nullptr}, {"num_paths", &a.agg_num_paths, nullptr, nullptr},
                              {"prolongation_type", &a.agg_prolongation_type, nullptr, &kAggInterp},
                              {"max_nnz_row", &a.agg_max_nnz_row, nullptr, nullptr}, {"trunc_factor", nullptr, &a.agg_trunc_factor, nullptr},
                              {"p12_max_elements", nullptr, &a.agg_P12_max_elements, nullptr},
                              {"p12_trunc_factor", nullptr, &a.agg_P12_trunc_factor, nullptr}});
      else if (k->key == "relaxation")
      {
         apply_fields(c, *k, {{"type", &a.relax_type, nullptr, &kRelax}, {"down_type", &a.down_type, nullptr, &kRelax},
                              {"up_type", &a.up_type, nullptr, &kRelax}, {"coarse_type", &a.coarse_type, nullptr, &kRelax},
                              {"down_sweeps", &a.down_sweeps, nullptr, nullptr}, {"up_sweeps", &a.up_sweeps, nullptr, nullptr},
                              {"coarse_sweeps", &a.coarse_sweeps, nullptr, nullptr}, {"num_sweeps", &a.num_sweeps, nullptr, nullptr},
                              {"order", &a.order, nullptr, nullptr}, {"points", &a.points, nullptr, &kPoints},
                              {"weight", nullptr, &a.weight, nullptr}, {"outer_weight", nullptr, &a.outer_weight, nullptr}},
                      {"chebyshev"});
         for (auto &q : k->kids)
            if (q->key == "points" && a.points != 0 && a.points != 1)
               c.fail(ERR_INVALID_VAL, "invalid value '" + q->val + "' for key 'points' (all / 0 or air / 1)");
         for (auto &q : k->kids)
            if (q->key == "chebyshev")
               apply_fields(c, *q, {{"order", &a.cheby_order, nullptr, nullptr}, {"eig_est", &a.cheby_eig_est, nullptr, nullptr},
                                    {"variant", &a.cheby_variant, nullptr, nullptr}, {"scale", &a.cheby_scale, nullptr, nullptr},
                                    {"fraction", nullptr, &a.cheby_fraction, nullptr}});
      }
      else if (k->key == "smoother")
      {
         apply_fields(c, *k, {{"type", &a.smooth_type, nullptr, &kSmoothType}, {"num_levels", &a.smooth_num_levels, nullptr, nullptr},
                              {"num_sweeps", &a.smooth_num_sweeps, nullptr, nullptr}},
                      {"fsai", "ilu"});
         for (auto &q : k->kids)
            if (q->key == "ilu") ilu_fields(c, *q, a.smooth_ilu);
            else if (q->key == "fsai") fsai_fields(c, *q, a.smooth_fsai);
      }
      else c.fail(ERR_INVALID_KEY, "unknown key '" + k->key + "' under 'amg'");
   }
}

// single-level aliases (reference src/internal/precon.c:255-288)
static void apply_alias(PreconArgs &p, const std::string &name)
{
   int t = (name == "jacobi") ? 0 : (name == "gauss-seidel") ? 3 : -1;
   if (t < 0) return;
   p.amg.max_levels    = 1;
   p.amg.relax_type    = t;
   p.amg.down_type     = t;
   p.amg.coarse_type   = t;
   p.amg.down_sweeps   = 1;
   p.amg.up_sweeps     = 0;
   p.amg.coarse_sweeps = 1;
}

static bool set_precon_method(Ctx &c, PreconArgs &p, const std::string &name)
{
   p = PreconArgs();
   p.method_name = name;
   if (name == "amg" || name == "boomeramg") p.method = 0;
   else if (name == "jacobi" || name == "gauss-seidel") { p.method = 0; apply_alias(p, name); }
   else if (name == "mgr") p.method = 1;
   else if (name == "ilu") p.method = 2;
   else if (name == "fsai") p.method = 3;
   else if (name == "ams") p.method = 4;
   else if (name == "ads") p.method = 5;
   else if (name == "schwarz") p.method = 6;
   else if (name == "none") p.method = 99;
   else { c.fail(ERR_INVALID_VAL, "unknown preconditioner '" + name + "'"); return false; }
   return true;
}

static const char *preset_text(const std::string &name)
{
   // built-in presets of the reference (src/internal/presets.c:17-33)
   if (name == "poisson") return "amg";
   if (name == "elasticity_2d") return "amg:\n  coarsening:\n    num_functions: 2\n    strong_th: 0.8";
   if (name == "elasticity_3d") return "amg:\n  coarsening:\n    num_functions: 3\n    strong_th: 0.8";
   return nullptr;
}

// preconditioner.reuse: value form (always | static | adaptive) or a block with enabled / frequency /
// linear_system_ids / per_timestep / type; same combinations rejected as in the reference
// (precon_reuse.c:2478-2550).  The adaptive policy and per_timestep need the reference's timestep files and
// solve-history model, which this build does not carry.
static void parse_reuse(Ctx &c, YNode &node, ReuseArgs &r)
{
   r = ReuseArgs();
   auto is_always = [](const std::string &v) { return lower(trim(v)) == "always"; };
   auto unsupported = [&](const char *what) { c.fail(ERR_INVALID_VAL, std::string("preconditioner.reuse ") + what + " is not implemented on MI355X (static policy only)"); };
   if (node.kids.empty())
   {
      const std::string v = lower(trim(node.val));
      if (v.empty()) return;
      if (is_always(v)) { r.enabled = 1; r.linear_system_ids = {0}; }
      else if (v == "static") r.enabled = 1;
      else if (v == "adaptive") unsupported("type: adaptive");
      else c.fail(ERR_INVALID_VAL, "Invalid preconditioner.reuse value: '" + node.val + "'");
      return;
   }
   bool seen_enabled = false, seen_freq = false, seen_ids = false, seen_ts = false, always = false;
   for (auto &k : node.kids)
   {
      if (k->key == "enabled") { r.enabled = to_int(c, *k, &kOnOff); seen_enabled = true; }
      else if (k->key == "frequency")
      {
         r.frequency = to_int(c, *k, nullptr);
         if (r.frequency < 0) c.fail(ERR_INVALID_VAL, "Invalid value for preconditioner.reuse.frequency: '" + k->val + "'");
         seen_freq = true;
      }
      else if (k->key == "linear_system_ids" || k->key == "linear_solver_ids")
      {
         std::string s = k->val;
         for (auto &q : k->kids) s += " " + (q->val.empty() ? q->key : q->val); // block sequence form
         for (char &ch : s)
            if (ch == '[' || ch == ']' || ch == ',') ch = ' ';
         std::istringstream is(s);
         std::string        tok;
         r.linear_system_ids.clear();
         while (is >> tok)
         {
            char *end = nullptr;
            long  v   = strtol(tok.c_str(), &end, 10);
            if (!end || *end) { c.fail(ERR_INVALID_VAL, "Failed to parse preconditioner.reuse.linear_system_ids"); break; }
            r.linear_system_ids.push_back((int)v);
         }
         if (r.linear_system_ids.empty()) c.fail(ERR_INVALID_VAL, "Failed to parse preconditioner.reuse.linear_system_ids");
         seen_ids = true;
      }
      else if (k->key == "per_timestep") { seen_ts = to_int(c, *k, &kOnOff) != 0; }
      else if (k->key == "type" || k->key == "policy")
      {
         const std::string v = lower(trim(k->val));
         if (is_always(v)) always = true;
         else if (v == "adaptive") unsupported("type: adaptive");
         else if (v != "static") c.fail(ERR_INVALID_VAL, "Invalid value for preconditioner.reuse.type: '" + k->val + "'");
      }
      else if (k->key == "guards" || k->key == "adaptive") unsupported(("block '" + k->key + "'").c_str());
      else c.fail(ERR_INVALID_KEY, "Unknown key under preconditioner.reuse: '" + k->key + "'");
   }
   if (!seen_enabled) r.enabled = 1;
   if (seen_ts) unsupported("per_timestep");
   if (always && !r.enabled) c.fail(ERR_INVALID_VAL, "preconditioner.reuse always cannot be combined with enabled: off");
   if (always && (seen_freq || seen_ids || seen_ts))
      c.fail(ERR_INVALID_VAL, "preconditioner.reuse always cannot be combined with frequency, linear_system_ids, or per_timestep");
   if (seen_ids && (seen_freq || seen_ts)) c.fail(ERR_INVALID_VAL, "preconditioner.reuse.linear_system_ids cannot be combined with frequency or per_timestep");
   if (always) r.linear_system_ids = {0};
   if (!r.enabled) { r.linear_system_ids.clear(); r.frequency = 0; }
}

static void parse_precon_body(Ctx &c, YNode &node, std::vector<PreconArgs> &variants);

uint32_t precon_from_text(const std::string &text, PreconArgs &out, std::string &message)
{
   Ctx   c;
   YNode root, holder;
   if (text.find(':') == std::string::npos && text.find('\n') == std::string::npos)
   {
      set_precon_method(c, out, lower(trim(text)));
      message = c.msg;
      return c.err;
   }
   uint32_t e = yaml_parse(text, root, message);
   if (e) return e;
   std::vector<PreconArgs> v;
   parse_precon_body(c, root, v);
   if (!v.empty()) out = v[0];
   message = c.msg;
   return c.err;
}

uint32_t solver_from_text(const std::string &text, KrylovArgs &out, std::string &message)
{
   Ctx   c;
   YNode root;
   if (text.find(':') == std::string::npos)
   {
      root.val = lower(trim(text));
      parse_solver(c, root, out);
   }
   else
   {
      uint32_t e = yaml_parse(text, root, message);
      if (e) return e;
      parse_solver(c, root, out);
   }
   message = c.msg;
   return c.err;
}

static void parse_precon_body(Ctx &c, YNode &node, std::vector<PreconArgs> &variants)
{
   for (auto &ch : node.kids)
   {
      if (ch->key == "reuse") continue; // parsed by args_from_yaml (parse_reuse)
      if (ch->key == "preset")
      {
         const char *t = preset_text(ch->val);
         if (!t) { c.fail(ERR_INVALID_VAL, "unknown preconditioner preset '" + ch->val + "'"); continue; }
         PreconArgs  p;
         std::string m;
         uint32_t    e = precon_from_text(t, p, m);
         if (e) c.fail(e, m);
         variants.push_back(p);
         continue;
      }
      if (ch->seq_item)
      { // "preconditioner: - amg: {...} - ilu: {...}" (what a list-valued include makes, examples/ex8-multi-2.yml): every item a full variant
         parse_precon_body(c, *ch, variants);
         continue;
      }
      PreconArgs p;
      if (!set_precon_method(c, p, ch->key)) continue;
      bool has_seq = false;
      for (auto &k : ch->kids) has_seq |= k->seq_item;
      if (has_seq)
      {
         for (auto &item : ch->kids)
         {
            if (!item->seq_item) { c.fail(ERR_YAML_TREE_INVALID, "mixing variants and plain keys under '" + ch->key + "'"); continue; }
            PreconArgs v = p;
            if (p.method == 0) amg_fields(c, *item, v.amg);
            else if (p.method == 2) ilu_fields(c, *item, v.ilu);
            else if (p.method == 1) mgr_fields(c, *item, v.mgr);
            else if (p.method == 6) schwarz_fields(c, *item, v.schwarz);
            else if (p.method == 4) ams_fields(c, *item, v.ams);
            else if (p.method == 3) fsai_fields(c, *item, v.fsai);
            variants.push_back(v);
         }
      }
      else
      {
         if (p.method == 0) amg_fields(c, *ch, p.amg);
         else if (p.method == 2) ilu_fields(c, *ch, p.ilu);
         else if (p.method == 1) mgr_fields(c, *ch, p.mgr);
         else if (p.method == 6) schwarz_fields(c, *ch, p.schwarz);
         else if (p.method == 4) ams_fields(c, *ch, p.ams);
         else if (p.method == 3) fsai_fields(c, *ch, p.fsai);
         variants.push_back(p);
      }
   }
}

uint32_t args_from_yaml(YNode &root, bool lib_mode, InputArgs &args, std::string &message)
{
   Ctx c;
   args.general.print_config_params = lib_mode ? 0 : 1;
   bool has_precon = false;
   for (auto &sec : root.kids)
   {
      if (sec->key == "general")
      {
         GeneralArgs &g = args.general;
         for (auto &k : sec->kids)
         {
            if (k->key == "name") g.name = k->val;
            else if (k->key == "statistics_filename") g.statistics_filename = k->val;
            else if (k->key == "warmup") g.warmup = to_int(c, *k, &kOnOff);
            else if (k->key == "statistics") g.statistics = to_int(c, *k, &kOnOff);
            else if (k->key == "print_config_params") g.print_config_params = to_int(c, *k, &kOnOff);
            else if (k->key == "use_millisec") g.use_millisec = to_int(c, *k, &kOnOff);
            else if (k->key == "num_repetitions") g.num_repetitions = to_int(c, *k, nullptr);
            else if (k->key == "exec_policy") g.exec_policy = to_int(c, *k, &kExec);
            else if (k->key == "device_lazy_init" || k->key == "use_vendor_spgemm" || k->key == "use_vendor_spmv" ||
                     k->key == "dev_pool_size" || k->key == "uvm_pool_size" || k->key == "host_pool_size" ||
                     k->key == "pinned_pool_size")
               ; // accepted: allocator / vendor-kernel knobs of the hypre backend have no meaning here
            else c.fail(ERR_INVALID_KEY, "unknown key '" + k->key + "' under 'general'");
         }
      }
      else if (sec->key == "linear_system")
      {
         LSArgs &l = args.ls;
         for (auto &k : sec->kids)
         {
            if (k->key == "dirname") l.dirname = k->val;
            else if (k->key == "matrix_filename") l.matrix_filename = k->val;
            else if (k->key == "matrix_basename") l.matrix_basename = k->val;
            else if (k->key == "precmat_filename") l.precmat_filename = k->val;
            else if (k->key == "rhs_filename") l.rhs_filename = k->val;
            else if (k->key == "rhs_basename") l.rhs_basename = k->val;
            else if (k->key == "x0_filename") l.x0_filename = k->val;
            else if (k->key == "xref_filename") l.xref_filename = k->val;
            else if (k->key == "sol_filename") l.sol_filename = k->val;
            else if (k->key == "dofmap_filename") l.dofmap_filename = k->val;
            else if (k->key == "digits_suffix") l.digits_suffix = to_int(c, *k, nullptr);
            else if (k->key == "init_suffix") l.init_suffix = to_int(c, *k, nullptr);
            else if (k->key == "last_suffix") l.last_suffix = to_int(c, *k, nullptr);
            else if (k->key == "init_guess_mode") l.init_guess_mode = to_int(c, *k, &kX0Mode);
            else if (k->key == "rhs_mode") l.rhs_mode = to_int(c, *k, &kRhsMode);
            else if (k->key == "type") l.type = to_int(c, *k, &kLsType);
            else if (k->key == "exec_policy") (void)to_int(c, *k, &kExec);
            else if (k->key == "precmat_basename") l.precmat_basename = k->val;
            else if (k->key == "dofmap_basename") l.dofmap_basename = k->val;
            else if (k->key == "set_suffix") l.set_suffix = int_list(c, *k, "set_suffix");
            else if (k->key == "sequence_filename")
               c.fail(ERR_INVALID_VAL, "linear_system.sequence_filename (single-file sequences) is not implemented on MI355X; use dirname / suffix directories");
            else if (k->key == "print_system" || k->key == "eigspec" || k->key == "dof_labels" || k->key == "timestep_filename" ||
                     k->key == "xref_basename")
               ; // diagnostics outside the solve path (dumps, spectra, reference solutions), symbolic label names
            else c.fail(ERR_INVALID_KEY, "unknown key '" + k->key + "' under 'linear_system'");
         }
         if (l.init_suffix >= 0 && l.last_suffix >= l.init_suffix) l.num_systems = l.last_suffix - l.init_suffix + 1;
         if (!l.set_suffix.empty()) l.num_systems = (int)l.set_suffix.size() + 1;
      }
      else if (sec->key == "solver") parse_solver(c, *sec, args.solver);
      else if (sec->key == "preconditioner")
      {
         has_precon = true;
         args.precon_variants.clear();
         if (!sec->val.empty() && sec->kids.empty())
         {
            PreconArgs p;
            if (set_precon_method(c, p, sec->val)) args.precon_variants.push_back(p);
         }
         else
         {
            for (auto &ch : sec->kids)
               if (ch->key == "reuse") parse_reuse(c, *ch, args.reuse);
            parse_precon_body(c, *sec, args.precon_variants);
         }
         if (args.precon_variants.empty()) c.fail(ERR_MISSING_PRECON, "preconditioner section names no preconditioner");
      }
      else
      { // the reference only looks its root sections up by name (args.c:235,261,300,982): anything else is left
        // unvisited and tolerated (its echo marks it "INVALID ENTRY"), e.g. the stray top-level 'ilu:' block of
        // examples/ex1b.yml.  Same here: ignored, with a note on stderr.
         fprintf(stderr, "hypredrive (MI355X): ignoring unknown root section '%s'\n", sec->key.c_str());
      }
   }
   if (!has_precon) c.fail(ERR_MISSING_PRECON, "missing 'preconditioner' section"); // reference args.c:981-989
   if (args.precon_variants.empty()) args.precon_variants.push_back(PreconArgs());
   args.has_precon     = has_precon;
   args.active_variant = 0;
   message             = c.msg;
   return c.err;
}

} // namespace hda
