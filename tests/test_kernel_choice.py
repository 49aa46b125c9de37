"""Which path kernel serves a renderer (csrc/vspg_kernel_choice.h): choose_kernel is a pure function of scene facts and four
environment variables, so the whole table is walked on a CPU.  tests/kernel_choice_table.cpp is compiled for the host and handed
one "facts|env" row per argument; it prints kernel_name(choose_kernel(facts, read_choice_env())) and arith_covered for each.

F0: homogeneous medium, no triangles, infinite lights, spheres or boundaries, uniform light sampler, all three grey flags true,
unguided, resampling, no tr_calc, no temperature.  G0: as F0 over a grid medium with medium_grey false; nvdb: G0 over NanoVDB.
KERNEL= stands for VSPG_KERNEL=, and so on."""
import os
import subprocess

import pytest

from conftest import ROOT

#        facts                          env                   name
NAMES = [("F0",                         "",                   "k_render_wave_wg3<HomogeneousMediumT<2,true>>"),
         ("F0",                         "WG_SCHED=2",         "k_render_wave_wg2<HomogeneousMediumT<2,true>>"),
         ("F0",                         "WG_SCHED=1",         "k_render_wave_wg<HomogeneousMediumT<2,true>>"),
         ("F0",                         "KERNEL=lane",        "k_render_wave<HomogeneousMedium>"),
         ("F0",                         "KERNEL=wf",          "k_render_wave<HomogeneousMedium>"),
         ("F0,null_zero=0",             "",                   "k_render_wave_wg3<HomogeneousMediumT<2,false>>"),
         ("F0,surfaces_grey=0",         "",                   "k_render_wave_wg3<HomogeneousMediumT<1,false>>"),
         ("F0,medium_grey=0",           "",                   "k_render_wave_wg3<HomogeneousMediumT<0,false>>"),
         ("F0,n_tris>0",                "",                   "k_render_wave_wg2<HomogeneousMedium>"),
         ("F0,n_tris>0",                "WG_SCHED=1",         "k_render_wave_wg2<HomogeneousMedium>"),
         ("F0,n_tris>0",                "KERNEL=lane",        "k_render_wave<HomogeneousMedium>"),
         ("F0,power",                   "",                   "k_render_wave_wg2<HomogeneousMedium>"),
         ("F0,guided",                  "",                   "k_render_wave_wg2<HomogeneousMediumT<2,true>,guided>"),
         ("F0,guided,training",         "",                   "k_render_wave_wg2<HomogeneousMediumT<2,true>,guided,train>"),
         ("F0,guided",                  "NO_GREY_GUIDED=1",   "k_render_wave_wg2<HomogeneousMedium,guided>"),
         ("F0,guided",                  "KERNEL=lane",        "k_render_wave<HomogeneousMediumT<2,true>,guided>"),
         ("F0,guided,rrguiding",        "",                   "k_render_wave<HomogeneousMediumT<2,true>,guided>"),
         ("F0,guided,n_tris>0",         "",                   "k_render_wave<HomogeneousMedium,guided>"),
         ("G0",                         "",                   "k_wf_dist_walk<GridMedium>"),
         ("G0,medium_grey=1",           "",                   "k_wf_dist_walk<GridMediumGrey>"),
         ("G0,boundaries",              "",                   "k_wf_walk<GridMedium>"),
         ("G0,guided",                  "",                   "k_wf_walk<GridMedium,guided>"),
         ("G0,guided",                  "WF_MERGED=0",        "k_wf_dist_walk<GridMedium,guided>"),
         ("G0,guided,training",         "",                   "k_wf_walk<GridMedium,guided,train>"),
         ("G0,not resampling",          "",                   "k_wf_segment_vertex<GridMedium>"),
         ("G0",                         "KERNEL=wg",          "k_render_wave_wg<GridMedium>"),
         ("G0,temperature",             "KERNEL=wg",          "k_render_wave<GridMedium>"),
         ("G0,tr_calc",                 "KERNEL=wg",          "k_render_wave<GridMedium>"),
         ("G0",                         "KERNEL=lane",        "k_render_wave<GridMedium>"),
         ("G0,medium_grey=1",           "KERNEL=lane",        "k_render_wave<GridMediumGrey>"),
         ("nvdb",                       "",                   "k_wf_dist_walk<NanoDenseMedium>"),
         ("nvdb",                       "KERNEL=wg",          "k_render_wave<NanoDenseMedium>"),
         ("nvdb,guided,training",       "",                   "k_wf_walk<NanoDenseMedium,guided,train>")]

#           facts               env           arith_covered
COVERED = [("F0",               "",           True),
           ("G0",               "",           True),
           ("F0",               "WG_SCHED=3", False),   # the cross-check kernels exist in exact arithmetic only: refused on presence,
           ("F0",               "WG_SCHED=",  False),   # ... of an empty value too
           ("F0",               "KERNEL=wg",  False),
           ("F0,guided",        "",           False),
           ("F0,n_tris>0",      "",           False),
           ("F0,tr_calc",       "",           False),
           ("G0,temperature",   "",           False),
           ("G0,not resampling", "",          False),
           ("nvdb",             "",           False)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(facts, env) -> (name, arith_covered) for every row of both lists, from one run of the driver."""
    exe = tmp_path_factory.mktemp("kernel_choice") / "kernel_choice_table"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "kernel_choice_table.cpp")])
    rows = [(f, e) for f, e, _ in NAMES] + [(f, e) for f, e, _ in COVERED] + [("F0", "KERNEL="), ("G0", "KERNEL=")]
    env = {k: v for k, v in os.environ.items() if not k.startswith("VSPG_")}
    out = subprocess.check_output([str(exe)] + ["%s|%s" % r for r in rows], env=env, text=True).splitlines()
    assert len(out) == len(rows)
    return {r: (line.split("\t")[0], line.split("\t")[1] == "1") for r, line in zip(rows, out)}


@pytest.mark.parametrize("facts,env,name", NAMES)
def test_kernel_name(table, facts, env, name):
    assert table[(facts, env)][0] == name


@pytest.mark.parametrize("facts,env,covered", COVERED)
def test_arith_covered(table, facts, env, covered):
    assert table[(facts, env)][1] is covered


@pytest.mark.parametrize("facts", ["F0", "G0"])
def test_an_empty_kernel_variable_counts_as_unset(table, facts):
    assert table[(facts, "KERNEL=")] == table[(facts, "")] and table[(facts, "")][1] is True


def test_header_is_plain_cxx():
    """No HIP header: include/vspg.h and the standard library only (the driver above is built by the host compiler alone)."""
    src = open(os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "vspg_kernel_choice.h")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert sorted(includes) == ['"../../include/vspg.h"', "<cstdlib>", "<string>"]
