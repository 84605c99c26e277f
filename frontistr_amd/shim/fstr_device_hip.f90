!> fistr1-side half of the device-resident Newton iteration (INTEGRATION.md section 5): the element loops of fstr_StiffMatrix
!> (fistr1/src/analysis/static/fstr_StiffMatrix.f90:18-212) and fstr_UpdateNewton (fstr_Update.f90:25-293) and the history update
!> of fstr_UpdateState (:296-345) forwarded to libfistr_hip, so that a Newton iteration of fstr_Newton
!> (fstr_solve_NonLinear.f90:29-167) moves vectors of 3*NP doubles between host and device instead of the 6.5 GB matrix:
!>   fstr_StiffMatrix  -> fx_nl_stiffness_at (unode, dunode up; the tangent stays on the device)
!>   fstr_AddBC        -> unchanged; its hecmw_mat_ass_bc calls are recorded (hecmw_hip_binding: fxb_defer_bc)
!>   solve_LINEQ       -> hecmw_solve -> fx_solve_device_matrix (B, X and the prescribed dofs up, X down)
!>   fstr_UpdateNewton -> fx_nl_update_at (dunode up, QFORCE down)
!>   fstr_UpdateState  -> fx_nl_commit + the quadrature-point history down (once per sub-step: results, restart)
!> Taken only for what the device kernels cover -- static analysis with NLGEOM, every element TYPE=361 with the B-bar formulation,
!> or (on one process) every element of one type of STF_C3 (TYPE=341, 342, 351, 352 or 362), or (on one process, with
!> HECMW_GPU_NL_MIXED=1) a mesh of several of these six types (fx_nl_init_groups, one group per elem_type_item entry), isotropic ELASTIC or Mises-elastoplastic
!> materials with isotropic hardening, no temperature / contact / MPC / spring / local coordinate system; fixed or automatic
!> increments (a cutback rolls the device's history back too, fsd_cutback); anything else runs the reference's own routines (kept,
!> renamed, in the same binary).
!> HECMW_GPU_ASSEMBLY=0 keeps the reference's element loops on the host for every deck; the tetrahedra are taken only with
!> Viscoelastic (!VISCOELASTIC, INFINITE / TOTALLAG) and NORTON creep (!CREEP, UPDATELAG) materials go there with HECMW_GPU_NL_VISCO=1:
!> ctime and tincr of every call reach the library through fx_nl_set_time, and the whole fstatus(:) of such points travels both ways.
!> HECMW_GPU_NL_TET=1, the five STF_C3 types with HECMW_GPU_NL_C3=1 (opt-in until their end-to-end time against the host loops
!> is on record).
module fstr_device_hip
  use iso_c_binding
  use hecmw
  use m_fstr
  use mMechGauss
  use mMaterial
  use m_step
  use hecmw_hip_binding
  implicit none
  private
  public :: fsd_stiffness, fsd_update_newton, fsd_update_state, fsd_active, fsd_report, fsd_cutback, fsd_set_time

  logical, save :: decided = .false., eligible = .false., ready = .false.
  ! linear static decks: the stiffness loop (fx_assemble_c3d8_sections) and the stress update (fx_update_c3d8_linear)
  logical, save :: lin_decided = .false., lin_eligible = .false., lin_ready = .false.
  type(c_ptr), save :: the_ctx_saved = c_null_ptr
  integer(c_int), save :: lin_elemopt = 0
  integer(c_int32_t), save :: lin_etype = 361      ! 361, or a type of STF_C3: 341 / 342 / 351 / 352 / 362 (fx_assemble_c3 / fx_update_c3_linear)
  real(c_double), allocatable, target, save :: lin_E(:), lin_nu(:)
  integer(c_int32_t), allocatable, target, save :: lin_emat(:)
  logical, save :: lin_thermal = .false.           ! !TEMPERATURE in a linear static deck (HECMW_GPU_THERMAL=1): fx_update_groups_linear_thermal
  real(c_double), allocatable, target, save :: lin_alpha(:)      ! M_EXAPNSION per material
  logical, save :: lin_mixed = .false.             ! several element types: fx_assemble_groups / fx_update_groups_linear
  ! (the stress update of a thermal deck goes through the groups too, lin_update_by_groups: a single type is one group there)
  type(fx_elem_group), allocatable, save :: lin_groups(:)    ! hecMESH%elem_type_index / elem_type_item as the library takes them
  integer(c_int32_t), save :: n_elem = 0
  integer(c_int32_t), save :: nl_etype = 361       ! nonlinear loop: 361 (B-bar), or a type of STF_C3 / UPDATE_C3 (fx_nl_init_type)
  integer, save :: nl_nq = 8                       ! its quadrature points per element
  logical, save :: nl_mixed = .false.              ! several of the six solid types (HECMW_GPU_NL_MIXED=1): fx_nl_init_groups
  logical, save :: nl_thermal = .false.            ! an NLGEOM deck with temperatures on the device (HECMW_GPU_NL_THERMAL=1): fx_nl_set_thermal
  logical, save :: nl_timed = .false.              ! viscoelastic or NORTON materials on the device (HECMW_GPU_NL_VISCO=1): fx_nl_set_time, the whole fstatus(:)
  integer(c_int32_t), save :: nl_hw = 0            ! components of their history per point (fx_nl_get_history)
  real(c_double), save :: nl_time = 0.d0, nl_tincr = 0.d0      ! ctime, tincr of the call in hand (fsd_set_time: the three forwarders)
  logical, save :: nl_fbar = .false.               ! the 361 sections are F-bar, all of them (HECMW_GPU_NL_FBAR=1): fx_nl_init_groups with elemopt 4
  integer, allocatable, save :: el_nq(:), el_p0(:) ! per element: its type's quadrature points, and the points of the elements before it
  integer, save :: n_pt = 0                        ! quadrature points of the mesh: the per-point arrays are flat over them, in hecMESH's element order
  real(c_double), allocatable, target, save :: tabs(:,:,:)       ! (2, ntab_max, n_mat): the MC_YIELD tables handed to the library
  ! what fx_nl_set_thermal was given (HECMW_GPU_NL_THERMAL=1): M_EXAPNSION, the MC_THEMOEXP / MC_ISOELASTIC tables, the initial condition
  real(c_double), allocatable, target, save :: th_alpha(:), th_atab(:,:,:), th_etab(:,:,:), th_init(:)
  integer(c_int32_t), allocatable, target, save :: th_arows(:), th_erows(:)
  type(c_ptr), allocatable, target, save :: th_aptr(:), th_eptr(:)
  real(c_double), allocatable, target, save :: b6(:,:)
  integer(c_int32_t), allocatable, target, save :: bi(:)

contains

  !> HECMW_GPU_REPORT=1: where each element loop ran and how long it took (wall clock), one line per call
  subroutine fsd_report(what, seconds)
    character(len=*), intent(in) :: what
    real(kind=kreal), intent(in) :: seconds
    character(len=8) :: env
    integer :: elen, estat
    logical, save :: asked = .false., on = .false.
    if (.not. asked) then
      asked = .true.
      call get_environment_variable('HECMW_GPU_REPORT', env, elen, estat)
      on = (estat == 0 .and. elen > 0 .and. env(1:1) == '1')
    endif
    if (on .and. hecmw_comm_get_rank() == 0) write(*,'(a,a,a,f10.3,a)') '### libfistr_hip: ', what, ': ', seconds, ' s'
  end subroutine fsd_report

  logical function fsd_active()
    fsd_active = ready
  end function fsd_active

  !> Is this run one the device kernels cover?  Decided once (the deck does not change during a run).
  logical function fsd_eligible(hecMESH, hecMAT, fstrSOLID)
    type(hecmwST_local_mesh), intent(in) :: hecMESH
    type(hecmwST_matrix), intent(in) :: hecMAT
    type(fstr_solid), intent(in) :: fstrSOLID
    character(len=8) :: env
    character(len=3) :: tname
    character(len=64) :: tnames
    integer :: elen, estat, i, icel, cid, nn, n_hyper, n_mises, n_yield, itype, n_bbar, n_fbar, n_visco, n_creep
    integer(c_int32_t) :: et
    logical :: opted, th
    character(len=32) :: tail
    if (decided) then
      fsd_eligible = eligible
      return
    endif
    decided = .true.
    eligible = .false.
    fsd_eligible = .false.
    call get_environment_variable('HECMW_GPU_ASSEMBLY', env, elen, estat)
    if (estat == 0 .and. elen > 0 .and. env(1:1) == '0') return
    call get_environment_variable('HECMW_GPU', env, elen, estat)
    if (estat == 0 .and. elen > 0 .and. env(1:1) == '0') return
    if (hecMAT%NDOF /= 3 .or. hecMESH%n_dof /= 3) return
    if (fstrPR%solution_type /= kstSTATIC .or. .not. fstrPR%nlgeom) return
    if (.not. fxb_on_gpu_path(hecMESH, hecMAT)) return                       ! the solve must run on the device too: same predicate as hecmw_solve (method, preconditioner, no MPC / contact)
    if (hecMESH%n_elem_type < 1) return
    nl_mixed = hecMESH%n_elem_type > 1
    if (nl_mixed) then      ! a mesh of several of the six solid types (fx_nl_init_groups): opt-in like the other nonlinear types, one process
      call get_environment_variable('HECMW_GPU_NL_MIXED', env, elen, estat)
      if (.not. (estat == 0 .and. elen > 0 .and. env(1:1) == '1')) return
      if (hecMESH%PETOT > 1) return
      if (hecMESH%n_elem_type > 16) return        ! (the report line names every type)
      do itype = 1, hecMESH%n_elem_type           ! any other type (371, beams, shells, 301) keeps the host loops
        et = int(hecMESH%elem_type_item(itype), c_int32_t)
        if (et /= 361 .and. c3_type_nodes(et) == 0) return
      enddo
      if (hecMESH%elem_type_index(hecMESH%n_elem_type) /= hecMESH%n_elem) return
    endif
    lin_etype = int(hecMESH%elem_type_item(1), c_int32_t)
    if (lin_etype /= 361 .and. c3_type_nodes(lin_etype) == 0) return             ! the nonlinear kernels: 361 B-bar and the types of STF_C3
    if (lin_etype /= 361 .and. hecMESH%PETOT > 1) return      ! decomposed meshes of these types: not yet on the device
    if (lin_etype /= 361 .and. .not. nl_mixed) then      ! these opt in: no end-to-end timing against the host loops has been recorded yet (DESIGN.md section 4)
      call get_environment_variable('HECMW_GPU_NL_C3', env, elen, estat)          ! the five types of STF_C3
      opted = (estat == 0 .and. elen > 0 .and. env(1:1) == '1')
      if (.not. opted .and. (lin_etype == 341 .or. lin_etype == 342)) then
        call get_environment_variable('HECMW_GPU_NL_TET', env, elen, estat)       ! the tetrahedra alone
        opted = (estat == 0 .and. elen > 0 .and. env(1:1) == '1')
      endif
      if (.not. opted) return
    endif
    nn = 8
    if (lin_etype /= 361) nn = c3_type_nodes(lin_etype)
    if (hecMESH%mpc%n_mpc > 0) return
    ! temperatures (`!TEMPERATURE`, also READRESULT: the array is made on the host): opt-in, one process, isotropic expansion, no
    ! temperature column in a yield table; the section orientations are refused below for every deck
    th = fstrSOLID%TEMP_ngrp_tot > 0 .or. fstrSOLID%TEMP_irres > 0
    if (th) then
      call get_environment_variable('HECMW_GPU_NL_THERMAL', env, elen, estat)
      if (.not. (estat == 0 .and. elen > 0 .and. env(1:1) == '1')) return
      if (hecMESH%PETOT > 1) return
      do i = 1, size(fstrSOLID%materials)
        if (fstrSOLID%materials(i)%mtype == -1) cycle
        if (.not. thermal_material_covered(fstrSOLID%materials(i))) return
      enddo
    endif
    if (fstrSOLID%SPRING_ngrp_tot > 0) return
    if (associated(fstrSOLID%contacts)) then
      if (size(fstrSOLID%contacts) > 0) return
    endif
    if (fstrSOLID%n_fix_mpc > 0) return
    ! (automatic incrementation, `!AUTOINC_PARAM`: fstr_cutback_save / _load roll the device's copy of the history back with the
    !  host's, shim/fstr_Cutback_hip.f90 -> fsd_cutback.  A run continued from a restart file: the history read from the file is what
    !  fsd_init pushes to the device at the first fstr_StiffMatrix, after fstr_read_restart, fstr_solve_NLGEOM.f90:70-76.)
    ! the formulation of the 361 elements: B-bar, or -- with HECMW_GPU_NL_FBAR=1 -- F-bar (`!SECTION, FORM361=FBAR`), the same for all
    ! of them: a mesh with sections of both keeps the host loops, as does any IC or FI section
    n_bbar = 0
    n_fbar = 0
    do i = 1, hecMESH%section%n_sect
      if (lin_etype == 361 .and. .not. nl_mixed) then
        if (fstrSOLID%sections(i)%elemopt361 == kel361BBAR) then
          n_bbar = n_bbar + 1
        else if (fstrSOLID%sections(i)%elemopt361 == kel361FBAR) then
          n_fbar = n_fbar + 1
        else
          return
        endif
      endif
      if (hecMESH%section%sect_orien_ID(i) > 0) return
    enddo
    if (nl_mixed) then      ! the node count per element, checked per type range; B-bar for the sections of the 361 elements
      do itype = 1, hecMESH%n_elem_type
        et = int(hecMESH%elem_type_item(itype), c_int32_t)
        nn = 8
        if (et /= 361) nn = c3_type_nodes(et)
        do icel = hecMESH%elem_type_index(itype-1) + 1, hecMESH%elem_type_index(itype)
          if (hecMESH%elem_node_index(icel) - hecMESH%elem_node_index(icel-1) /= nn) return
          if (et == 361) then
            if (fstrSOLID%sections(hecMESH%section_ID(icel))%elemopt361 == kel361BBAR) then
              n_bbar = n_bbar + 1
            else if (fstrSOLID%sections(hecMESH%section_ID(icel))%elemopt361 == kel361FBAR) then
              n_fbar = n_fbar + 1
            else
              return
            endif
          endif
          cid = hecMESH%section%sect_mat_ID_item(hecMESH%section_ID(icel))
          if (.not. associated(fstrSOLID%elements(icel)%gausses(1)%pMaterial, fstrSOLID%materials(cid))) return
        enddo
      enddo
    else
      do icel = 1, hecMESH%n_elem
        if (hecMESH%elem_node_index(icel) - hecMESH%elem_node_index(icel-1) /= nn) return
        cid = hecMESH%section%sect_mat_ID_item(hecMESH%section_ID(icel))
        if (.not. associated(fstrSOLID%elements(icel)%gausses(1)%pMaterial, fstrSOLID%materials(cid))) return
      enddo
    endif
    nl_fbar = n_fbar > 0
    if (nl_fbar) then
      ! F-bar decks opt in: no end-to-end time against the host loops is on record (DESIGN.md section 7)
      if (n_bbar > 0) return
      if (hecMESH%PETOT > 1) return
      call get_environment_variable('HECMW_GPU_NL_FBAR', env, elen, estat)
      if (.not. (estat == 0 .and. elen > 0 .and. env(1:1) == '1')) return
      ! Update_C3D8Fbar's UPDATELAG branch reads a local array it never assigned (static_LIB_Fbar.f90:600-602): no material of an
      ! F-bar section may be UPDATELAG (`!ELASTIC, CAUCHY`, the default of `!PLASTIC`)
      do icel = 1, hecMESH%n_elem
        if (hecMESH%elem_type(icel) /= 361) cycle
        if (fstrSOLID%elements(icel)%gausses(1)%pMaterial%nlgeom_flag == UPDATELAG) return
      enddo
    endif
    n_hyper = 0
    n_mises = 0
    n_yield = 0
    n_visco = 0
    n_creep = 0
    do i = 1, size(fstrSOLID%materials)
      if (.not. material_covered(fstrSOLID%materials(i))) return
      if (is_hyperelastic(fstrSOLID%materials(i)%mtype)) n_hyper = n_hyper + 1
      if (fstrSOLID%materials(i)%mtype == VISCOELASTIC) n_visco = n_visco + 1
      if (fstrSOLID%materials(i)%mtype == NORTON) n_creep = n_creep + 1
      if (fstrSOLID%materials(i)%mtype /= -1 .and. isElastoplastic(fstrSOLID%materials(i)%mtype)) then
        n_mises = n_mises + 1      ! every elastoplastic material, whatever its yield function: what sets MatlMatrix's saved flag
        if (getYieldFunction(fstrSOLID%materials(i)%mtype) /= 0) n_yield = n_yield + 1
      endif
    enddo
    if (n_yield > 0) then
      ! YIELD=MOHR-COULOMB / DRUCKER-PRAGER decks opt in: no end-to-end time against the host loops is on record (DESIGN.md section 7)
      call get_environment_variable('HECMW_GPU_NL_YIELD', env, elen, estat)
      if (.not. (estat == 0 .and. elen > 0 .and. env(1:1) == '1')) return
    endif
    if (n_hyper > 0) then
      ! !HYPERELASTIC decks opt in (no end-to-end time against the host loops is on record); beside a plastic material they keep the
      ! host loops: after the first plastic update MatlMatrix's saved flag sends every material to calElasticMatrix (DESIGN.md section 8)
      if (n_mises > 0) return
      call get_environment_variable('HECMW_GPU_NL_HYPER', env, elen, estat)
      if (.not. (estat == 0 .and. elen > 0 .and. env(1:1) == '1')) return
    endif
    if (n_visco + n_creep > 0) then
      ! !VISCOELASTIC / !CREEP decks opt in: no end-to-end time against the host loops is on record (DESIGN.md section 7).  Any
      ! temperature in the deck keeps the host loops (fx_nl_set_thermal refuses these materials), a NORTON material beside a
      ! hyperelastic one too (its first stress update sets MatlMatrix's saved flag), and a decomposed mesh
      if (th) return
      if (n_creep > 0 .and. n_hyper > 0) return
      if (hecMESH%PETOT > 1) return
      call get_environment_variable('HECMW_GPU_NL_VISCO', env, elen, estat)
      if (.not. (estat == 0 .and. elen > 0 .and. env(1:1) == '1')) return
    endif
    nl_timed = n_visco + n_creep > 0
    eligible = .true.
    fsd_eligible = .true.
    nl_thermal = th
    tail = ''
    if (th) tail = ', thermal'
    if (n_visco > 0) tail = trim(tail)//', viscoelastic'
    if (n_creep > 0) tail = trim(tail)//', creep'
    nl_etype = lin_etype
    nl_nq = 8
    if (nl_etype /= 361) nl_nq = c3_type_points(nl_etype)
    if (nl_mixed) then      ! the types in hecMESH's order: TYPE=341+351+361
      write(tname, '(i3)') nl_etype
      tnames = tname
      do itype = 2, hecMESH%n_elem_type
        write(tname, '(i3)') hecMESH%elem_type_item(itype)
        tnames = trim(tnames)//'+'//tname
      enddo
      if (hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: stiffness assembly and stress update on the device (TYPE='//trim(tnames)//'); '// &
        'HECMW_GPU_ASSEMBLY=0 keeps them on the host'//trim(tail)
      if (nl_fbar .and. hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: the TYPE=361 sections are F-bar (HECMW_GPU_NL_FBAR=1)'
      if (n_hyper > 0 .and. hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: hyperelastic materials on the device (HECMW_GPU_NL_HYPER=1)'
      if (n_yield > 0 .and. hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: Mohr-Coulomb / Drucker-Prager materials on the device (HECMW_GPU_NL_YIELD=1)'
      return
    endif
    if (nl_etype /= 361) then
      write(tname, '(i3)') nl_etype
      if (hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: stiffness assembly and stress update on the device (TYPE='//tname//'); '// &
        'HECMW_GPU_ASSEMBLY=0 keeps them on the host'//trim(tail)
      if (n_hyper > 0 .and. hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: hyperelastic materials on the device (HECMW_GPU_NL_HYPER=1)'
      if (n_yield > 0 .and. hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: Mohr-Coulomb / Drucker-Prager materials on the device (HECMW_GPU_NL_YIELD=1)'
      return
    endif
    if (nl_fbar) then
      if (hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: stiffness assembly and stress update on the device (TYPE=361 F-bar); '// &
        'HECMW_GPU_ASSEMBLY=0 keeps them on the host'//trim(tail)
    else
      if (hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: stiffness assembly and stress update on the device (TYPE=361 B-bar); '// &
        'HECMW_GPU_ASSEMBLY=0 keeps them on the host'//trim(tail)
    endif
    if (n_hyper > 0 .and. hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: hyperelastic materials on the device (HECMW_GPU_NL_HYPER=1)'
    if (n_yield > 0 .and. hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: Mohr-Coulomb / Drucker-Prager materials on the device (HECMW_GPU_NL_YIELD=1)'
  end function fsd_eligible

  !> Where fstr_UpdateNewton of an eligible linear static deck runs.  HECMW_GPU_UPDATE=0: the host, =1: the device.  Unset: the
  !> device for 361, 341 and 342; the host for 351, 352 and 362, whose device update was measured slower than the reference's
  !> loop on 16 threads at a million elements (the copy of 2 x 6 x nq doubles per element back into gausses(:) outweighs the
  !> kernel; DESIGN.md section 4), so these types opt in.
  logical function lin_update_on_device()
    character(len=8) :: env
    integer :: elen, estat
    call get_environment_variable('HECMW_GPU_UPDATE', env, elen, estat)
    if (estat == 0 .and. elen > 0) then
      lin_update_on_device = env(1:1) /= '0'
    else if (lin_mixed) then
      lin_update_on_device = .false.      ! a mesh of several types: the host unless asked for (DESIGN.md section 4, "mixed meshes")
    else
      lin_update_on_device = .not. (lin_etype == 351 .or. lin_etype == 352 .or. lin_etype == 362)
    endif
  end function lin_update_on_device

  !> Does the stress update go through the groups entry points?  A mesh of several types, and any thermal deck: the thermal
  !> update has no single-type entry point, so a single type is one group there.  (The assembly of a single-type thermal deck
  !> stays with the single-type entry points: the stiffness knows no temperature.)
  logical function lin_update_by_groups()
    lin_update_by_groups = lin_mixed .or. lin_thermal
  end function lin_update_by_groups

  !> Nodes per element of the types STF_C3 / UPDATE_C3 serve on the device beside 361; 0: not one of them.
  pure integer function c3_type_nodes(etype)
    integer(c_int32_t), intent(in) :: etype
    select case (etype)
      case (341); c3_type_nodes = 4
      case (342); c3_type_nodes = 10
      case (351); c3_type_nodes = 6
      case (352); c3_type_nodes = 15
      case (362); c3_type_nodes = 20
      case default; c3_type_nodes = 0
    end select
  end function c3_type_nodes

  !> Their quadrature points per element (NumOfQuadPoints).
  pure integer function c3_type_points(etype)
    integer(c_int32_t), intent(in) :: etype
    select case (etype)
      case (341); c3_type_points = 1
      case (342); c3_type_points = 4
      case (351); c3_type_points = 2
      case (352); c3_type_points = 9
      case (362); c3_type_points = 27
      case default; c3_type_points = 0
    end select
  end function c3_type_points

  !> Linear static analysis (`!SOLUTION, TYPE=STATIC`, small strain) of TYPE=361 elements with isotropic ELASTIC materials: the
  !> element loop of fstr_StiffMatrix runs on the device -- STF_C3D8IC (the default of 361), STF_C3D8Bbar or STF_C3, whichever
  !> `!SECTION ... ELEMOPT361` selects, the same for every section -- and the matrix stays there for hecmw_solve; fstr_UpdateNewton
  !> (strains, stresses, QFORCE from the solution vector) runs there too (fsd_update_newton_linear).  A mesh of tetrahedra only,
  !> TYPE=341 or 342, of wedges only, TYPE=351 or 352, or of 20-node hexahedra only, TYPE=362 (STF_C3 / UPDATE_C3,
  !> fstr_StiffMatrix.f90:134-144, fstr_Update.f90:182-189), is covered the same way under
  !> the same conditions, ELEMOPT361 aside; a decomposed mesh of these types (PETOT > 1) keeps the host loops.  A mesh of several
  !> of the six types (hecMESH%n_elem_type > 1, one rank) is covered through fx_assemble_groups, one group per entry of
  !> elem_type_item; any other type in the mesh (371, beams, shells, link elements) keeps the host loops.
  logical function fsd_eligible_linear(hecMESH, hecMAT, fstrSOLID)
    type(hecmwST_local_mesh), intent(in) :: hecMESH
    type(hecmwST_matrix), intent(in) :: hecMAT
    type(fstr_solid), intent(in) :: fstrSOLID
    character(len=8) :: env
    integer :: elen, estat, i, icel, cid, opt, nn, itype
    integer(c_int32_t) :: et
    character(len=3) :: tname
    character(len=64) :: tnames
    character(len=9) :: suffix
    logical :: has361
    if (lin_decided) then
      fsd_eligible_linear = lin_eligible
      return
    endif
    lin_decided = .true.
    lin_eligible = .false.
    fsd_eligible_linear = .false.
    call get_environment_variable('HECMW_GPU_ASSEMBLY', env, elen, estat)
    if (estat == 0 .and. elen > 0 .and. env(1:1) == '0') return
    call get_environment_variable('HECMW_GPU', env, elen, estat)
    if (estat == 0 .and. elen > 0 .and. env(1:1) == '0') return
    if (hecMAT%NDOF /= 3 .or. hecMESH%n_dof /= 3) return
    if (fstrPR%solution_type /= kstSTATIC .or. fstrPR%nlgeom) return
    if (.not. fxb_on_gpu_path(hecMESH, hecMAT)) return
    if (hecMESH%n_elem_type < 1) return
    lin_mixed = hecMESH%n_elem_type > 1
    if (lin_mixed .and. hecMESH%PETOT > 1) return               ! decomposed mixed meshes: not yet on the device
    if (lin_mixed .and. hecMESH%n_elem_type > 16) return        ! (the report line names every type)
    has361 = .false.
    do itype = 1, hecMESH%n_elem_type
      et = int(hecMESH%elem_type_item(itype), c_int32_t)
      if (et /= 361 .and. c3_type_nodes(et) == 0) return
      if (et == 361) has361 = .true.
    enddo
    lin_etype = int(hecMESH%elem_type_item(1), c_int32_t)
    if (lin_etype /= 361 .and. hecMESH%PETOT > 1) return      ! decomposed meshes of these types: not yet on the device
    if (hecMESH%mpc%n_mpc > 0) return
    lin_thermal = fstrSOLID%TEMP_ngrp_tot > 0 .or. fstrSOLID%TEMP_irres > 0
    if (lin_thermal) then      ! thermal strains enter the element routines: fx_update_groups_linear_thermal has them, one constant
      ! isotropic expansion coefficient per material.  No end-to-end timing against the host loops has been recorded yet, so
      ! thermal decks opt in (DESIGN.md section 7); one rank only.
      call get_environment_variable('HECMW_GPU_THERMAL', env, elen, estat)
      if (.not. (estat == 0 .and. elen > 0 .and. env(1:1) == '1')) return
      if (hecMESH%PETOT > 1) return
    endif
    if (fstrSOLID%SPRING_ngrp_tot > 0) return
    if (associated(fstrSOLID%contacts)) then
      if (size(fstrSOLID%contacts) > 0) return
    endif
    if (fstrSOLID%n_fix_mpc > 0) return
    opt = -1
    do i = 1, hecMESH%section%n_sect
      if (opt == -1) opt = fstrSOLID%sections(i)%elemopt361
      if (has361 .and. fstrSOLID%sections(i)%elemopt361 /= opt) return
      if (hecMESH%section%sect_orien_ID(i) > 0) return
    enddo
    if (has361) then                 ! ELEMOPT361 selects the 361 formulation only
      select case (opt)
        case (kel361IC);   lin_elemopt = 1
        case (kel361BBAR); lin_elemopt = 2
        case (kel361FI);   lin_elemopt = 3
        case default; return
      end select
    endif
    do itype = 1, hecMESH%n_elem_type      ! the node count per element, checked per type range
      et = int(hecMESH%elem_type_item(itype), c_int32_t)
      nn = 8
      if (et /= 361) nn = c3_type_nodes(et)
      do icel = hecMESH%elem_type_index(itype-1) + 1, hecMESH%elem_type_index(itype)
        if (hecMESH%elem_node_index(icel) - hecMESH%elem_node_index(icel-1) /= nn) return
        cid = hecMESH%section%sect_mat_ID_item(hecMESH%section_ID(icel))
        if (.not. associated(fstrSOLID%elements(icel)%gausses(1)%pMaterial, fstrSOLID%materials(cid))) return
      enddo
    enddo
    if (hecMESH%elem_type_index(hecMESH%n_elem_type) /= hecMESH%n_elem) return
    do i = 1, size(fstrSOLID%materials)
      if (fstrSOLID%materials(i)%mtype == -1) cycle
      if (fstrSOLID%materials(i)%mtype /= ELASTIC) return
      if (fstrSOLID%materials(i)%nlgeom_flag /= INFINITE) return
      if (fetch_TableRow(MC_ISOELASTIC, fstrSOLID%materials(i)%dict) > 1) return     ! temperature-dependent constants
      if (lin_thermal) then
        if (fetch_TableRow(MC_THEMOEXP, fstrSOLID%materials(i)%dict) > 1) return     ! a table of expansion coefficients
        if (fetch_TableRow(MC_ORTHOEXP, fstrSOLID%materials(i)%dict) > 0) return     ! orthotropic expansion
      endif
    enddo
    lin_eligible = .true.
    fsd_eligible_linear = .true.
    write(tname, '(i3)') lin_etype
    tnames = tname
    do itype = 2, hecMESH%n_elem_type      ! a mixed mesh: the types in mesh order, TYPE=361+351+341
      write(tname, '(i3)') hecMESH%elem_type_item(itype)
      tnames = trim(tnames)//'+'//tname
    enddo
    suffix = ''
    if (lin_thermal) suffix = ', thermal'
    if (hecMESH%my_rank == 0) write(*,'(a)') '### libfistr_hip: stiffness assembly on the device (linear static, TYPE='//trim(tnames)//'); '// &
      'HECMW_GPU_ASSEMBLY=0 keeps it on the host'//trim(suffix)
  end function fsd_eligible_linear

  subroutine fsd_init_linear(hecMESH, hecMAT, fstrSOLID)
    type(hecmwST_local_mesh), intent(in), target :: hecMESH
    type(hecmwST_matrix), intent(in), target :: hecMAT
    type(fstr_solid), intent(in) :: fstrSOLID
    type(c_ptr) :: ctx
    type(fx_matrix_view) :: mv
    type(fx_comm_view) :: cv
    integer(c_int) :: ierr
    integer :: i, icel, nmat, itype, first
    ctx = fxb_context(hecMESH)
    call fxb_ensure_transport(hecMESH, 3)
    call fxb_views(hecMESH, hecMAT, mv, cv)
    mv%D = c_null_ptr; mv%AL = c_null_ptr; mv%AU = c_null_ptr; mv%B = c_null_ptr; mv%X = c_null_ptr   ! profile only
    ierr = fx_upload(ctx, mv, cv, FX_UP_PROFILE)
    if (ierr /= 0) call fsd_fail('profile upload')
    nmat = size(fstrSOLID%materials)
    if (allocated(lin_E)) deallocate(lin_E, lin_nu, lin_emat)
    allocate(lin_E(nmat), lin_nu(nmat), lin_emat(hecMESH%n_elem))
    lin_E = 1.d0; lin_nu = 0.d0
    do i = 1, nmat
      if (fstrSOLID%materials(i)%mtype == -1) cycle
      lin_E(i) = fstrSOLID%materials(i)%variables(M_YOUNGS)
      lin_nu(i) = fstrSOLID%materials(i)%variables(M_POISSON)
    enddo
    if (lin_thermal) then
      if (allocated(lin_alpha)) deallocate(lin_alpha)
      allocate(lin_alpha(nmat))
      lin_alpha = 0.d0
      do i = 1, nmat
        if (fstrSOLID%materials(i)%mtype == -1) cycle
        lin_alpha(i) = fstrSOLID%materials(i)%variables(M_EXAPNSION)
      enddo
    endif
    do icel = 1, hecMESH%n_elem
      lin_emat(icel) = hecMESH%section%sect_mat_ID_item(hecMESH%section_ID(icel))
    enddo
    if (lin_update_by_groups()) then     ! elem_node_item holds the elements type by type: a group is a pointer into it (and into lin_emat)
      if (allocated(lin_groups)) deallocate(lin_groups)
      allocate(lin_groups(hecMESH%n_elem_type))
      do itype = 1, hecMESH%n_elem_type
        first = hecMESH%elem_type_index(itype-1) + 1
        lin_groups(itype)%etype = int(hecMESH%elem_type_item(itype), c_int32_t)
        lin_groups(itype)%elemopt = max(lin_elemopt, 1)
        lin_groups(itype)%n_elem = int(hecMESH%elem_type_index(itype) - hecMESH%elem_type_index(itype-1), c_int32_t)
        lin_groups(itype)%conn = c_null_ptr
        lin_groups(itype)%elem_mat = c_null_ptr
        if (lin_groups(itype)%n_elem > 0) then
          lin_groups(itype)%conn = c_loc(hecMESH%elem_node_item(hecMESH%elem_node_index(first-1) + 1))
          lin_groups(itype)%elem_mat = c_loc(lin_emat(first))
        endif
      enddo
    endif
    lin_ready = .true.
  end subroutine fsd_init_linear

  logical function material_covered(m)
    type(tMaterial), intent(in) :: m
    type(DICT_DATA), pointer :: tbl
    logical :: ierr_l
    integer :: k
    material_covered = .false.
    if (m%mtype == -1) then            ! a slot of fstrSOLID%materials no section refers to (initMaterial never ran): ignored
      material_covered = .true.
      return
    endif
    if (m%nlgeom_flag /= INFINITE .and. m%nlgeom_flag /= TOTALLAG .and. m%nlgeom_flag /= UPDATELAG) return
    if (m%mtype == ELASTIC) then
      material_covered = .true.
    else if (isElastoplastic(m%mtype)) then
      if (isKinematicHarden(m%mtype)) return
      if (getYieldFunction(m%mtype) == 1 .or. getYieldFunction(m%mtype) == 2) then
        ! Mohr-Coulomb, Drucker-Prager: the card forces linear hardening (fstr_ctrl_material.f90:452); the constants at which the
        ! return would stop are left to the host loops
        if (getHardenType(m%mtype) /= 0) return
        if (getYieldFunction(m%mtype) == 1 .and. cos(m%variables(M_PLCONST3)) == 0.d0) return
        if (getYieldFunction(m%mtype) == 2 .and. m%variables(M_PLCONST4) == 0.d0) return
        material_covered = .true.
        return
      endif
      if (getYieldFunction(m%mtype) /= 0) return         ! Mises
      if (getHardenType(m%mtype) < 0 .or. getHardenType(m%mtype) > 3) return
      material_covered = .true.
    else if (m%mtype == VISCOELASTIC) then
      ! the plain card only (a !TRS card makes the mtype VISCOELASTIC + 1 / + 2: host loops), INFINITE or TOTALLAG, no DEPENDENCIES
      ! column, no relaxation time of zero
      if (m%nlgeom_flag /= INFINITE .and. m%nlgeom_flag /= TOTALLAG) return
      call fetch_Table(MC_VISCOELASTIC, m%dict, tbl, ierr_l)
      if (ierr_l) return
      ! (the card makes its table with ndepends = 1 whatever DEPENDENCIES says, fstr_ctrl_material.f90:302: a temperature column shows
      ! as a third column)
      if (tbl%tbcol /= 2 .or. tbl%tbrow < 1) return
      do k = 1, tbl%tbrow
        if (tbl%tbval(2, k) == 0.d0) return
      enddo
      material_covered = .true.
    else if (m%mtype == NORTON) then
      ! UPDATELAG (the card's default), no DEPENDENCIES, a time exponent above -1
      if (m%nlgeom_flag /= UPDATELAG) return
      call fetch_Table(MC_NORTON, m%dict, tbl, ierr_l)
      if (ierr_l) return
      if (tbl%ndepends /= 0 .or. tbl%tbrow /= 1) return
      if (.not. (tbl%tbval(3, 1) > -1.d0)) return
      material_covered = .true.
    else if (is_hyperelastic(m%mtype)) then
      ! total Lagrange only (`CAUCHY` -> UPDATELAG is another algorithm in the reference).  A card with a DEPENDENCIES table never gets
      ! here: fstr_ctrl_get_HYPERELASTIC reads data only when DEPENDENCIES is 0 and returns -1 otherwise, so set-up stops on such a deck.
      if (m%nlgeom_flag /= TOTALLAG) return
      if (m%variables(M_PLCONST3) == 0.d0) return
      if (m%mtype == ARRUDABOYCE .and. m%variables(M_PLCONST2) == 0.d0) return
      material_covered = .true.
    endif
  end function material_covered

  !> What the device's thermal strain serves of a material: isotropic expansion (no MC_ORTHOEXP), MC_THEMOEXP and MC_ISOELASTIC
  !> constant or with one dependency, and no temperature column in MC_YIELD
  logical function thermal_material_covered(m)
    type(tMaterial), intent(in) :: m
    type(DICT_DATA), pointer :: tbl
    logical :: miss
    thermal_material_covered = .false.
    if (fetch_TableRow(MC_ORTHOEXP, m%dict) > 0) return
    call fetch_Table(MC_THEMOEXP, m%dict, tbl, miss)
    if (.not. miss) then
      if (tbl%ndepends > 1) return
    endif
    call fetch_Table(MC_ISOELASTIC, m%dict, tbl, miss)
    if (.not. miss) then
      if (tbl%ndepends > 1) return
      if (tbl%ndepends == 1 .and. is_hyperelastic(m%mtype)) return
    endif
    call fetch_Table(MC_YIELD, m%dict, tbl, miss)
    if (.not. miss) then
      if (isElastoplastic(m%mtype) .and. getHardenType(m%mtype) == 1) then
        if (tbl%ndepends > 1) return      ! MULTILINEAR: (yield stress, plastic strain) and nothing more
      else if (tbl%ndepends > 0) then
        return
      endif
    endif
    thermal_material_covered = .true.
  end function thermal_material_covered

  !> fx_nl_set_thermal from M_EXAPNSION, MC_THEMOEXP, MC_ISOELASTIC, ref_temp and the initial condition; last_temp as the host has it
  subroutine fsd_init_thermal(ctx, hecMESH, fstrSOLID)
    type(c_ptr), intent(in) :: ctx
    type(hecmwST_local_mesh), intent(in) :: hecMESH
    type(fstr_solid), intent(inout), target :: fstrSOLID
    type(fx_nl_thermal_view) :: tv
    type(DICT_DATA), pointer :: tbl
    logical :: miss
    integer(c_int) :: ierr
    integer :: i, j, nmat, nrow
    nmat = size(fstrSOLID%materials)
    nrow = 1
    do i = 1, nmat
      if (fstrSOLID%materials(i)%mtype == -1) cycle
      nrow = max(nrow, fetch_TableRow(MC_THEMOEXP, fstrSOLID%materials(i)%dict), fetch_TableRow(MC_ISOELASTIC, fstrSOLID%materials(i)%dict))
    enddo
    if (allocated(th_alpha)) deallocate(th_alpha, th_atab, th_etab, th_arows, th_erows, th_aptr, th_eptr, th_init)
    allocate(th_alpha(nmat), th_atab(2, nrow, nmat), th_etab(3, nrow, nmat), th_arows(nmat), th_erows(nmat), th_aptr(nmat), th_eptr(nmat), &
             th_init(hecMESH%n_node))
    th_alpha = 0.d0; th_arows = 0; th_erows = 0
    do i = 1, nmat
      th_aptr(i) = c_null_ptr; th_eptr(i) = c_null_ptr
      if (fstrSOLID%materials(i)%mtype == -1) cycle
      th_alpha(i) = fstrSOLID%materials(i)%variables(M_EXAPNSION)
      call fetch_Table(MC_THEMOEXP, fstrSOLID%materials(i)%dict, tbl, miss)      ! rows (alpha, T) as the reference holds them
      if (.not. miss) then
        if (tbl%ndepends == 1) then
          th_arows(i) = tbl%tbrow
          th_atab(1:2, 1:tbl%tbrow, i) = tbl%tbval(1:2, 1:tbl%tbrow)
          th_aptr(i) = c_loc(th_atab(1, 1, i))
        else
          th_alpha(i) = tbl%tbval(1, 1)
        endif
      endif
      call fetch_Table(MC_ISOELASTIC, fstrSOLID%materials(i)%dict, tbl, miss)    ! rows (E, nu, T)
      if (.not. miss) then
        if (tbl%ndepends == 1) then
          th_erows(i) = tbl%tbrow
          th_etab(1:3, 1:tbl%tbrow, i) = tbl%tbval(1:3, 1:tbl%tbrow)
          th_eptr(i) = c_loc(th_etab(1, 1, i))
        endif
      endif
    enddo
    tv%ref_temp = REF_TEMP
    tv%temp_init = c_null_ptr
    if (hecMESH%hecmw_flag_initcon == 1) then      ! tt0 of fstr_Update.f90:97-98
      do j = 1, hecMESH%n_node
        th_init(j) = hecMESH%node_init_val_item(j)
      enddo
      tv%temp_init = c_loc(th_init(1))
    endif
    tv%alpha = c_loc(th_alpha(1))
    tv%alpha_tab = c_loc(th_aptr(1)); tv%alpha_rows = c_loc(th_arows(1))
    tv%elastic_tab = c_loc(th_eptr(1)); tv%elastic_rows = c_loc(th_erows(1))
    ierr = fx_nl_set_thermal(ctx, tv)
    if (ierr /= 0) call fsd_fail('fx_nl_set_thermal')
    ierr = fx_nl_set_last_temp(ctx, fstrSOLID%last_temp)      ! (fstr_UpdateState at the start of the step has already run)
    if (ierr /= 0) call fsd_fail('fx_nl_set_last_temp')
    ierr = fx_nl_set_temperature(ctx, fstrSOLID%temperature)
    if (ierr /= 0) call fsd_fail('fx_nl_set_temperature')
  end subroutine fsd_init_thermal

  logical function is_hyperelastic(mtype)
    integer, intent(in) :: mtype
    is_hyperelastic = (mtype == NEOHOOKE .or. mtype == MOONEYRIVLIN .or. mtype == ARRUDABOYCE)
  end function is_hyperelastic

  !> First use: profile, mesh, materials and the current quadrature-point history go to the device.
  subroutine fsd_init(hecMESH, hecMAT, fstrSOLID)
    type(hecmwST_local_mesh), intent(in), target :: hecMESH
    type(hecmwST_matrix), intent(in), target :: hecMAT
    type(fstr_solid), intent(inout), target :: fstrSOLID
    type(c_ptr) :: ctx
    type(fx_matrix_view) :: mv
    type(fx_comm_view) :: cv
    type(fx_mesh_view) :: mesh
    type(fx_material_view), allocatable :: mats(:)
    integer(c_int32_t), allocatable, target :: emat(:)
    type(fx_elem_group), allocatable :: groups(:)
    type(DICT_DATA), pointer :: tbl
    logical :: ierr_l
    integer(c_int) :: ierr
    integer :: i, nmat, ntmax, nt, icel, itype, first, nq
    ctx = fxb_context(hecMESH)
    call fxb_ensure_transport(hecMESH, 3)
    call fxb_views(hecMESH, hecMAT, mv, cv)
    mv%D = c_null_ptr; mv%AL = c_null_ptr; mv%AU = c_null_ptr; mv%B = c_null_ptr; mv%X = c_null_ptr   ! profile only
    ierr = fx_upload(ctx, mv, cv, FX_UP_PROFILE)
    if (ierr /= 0) call fsd_fail('profile upload')
    n_elem = hecMESH%n_elem
    mesh%n_node = hecMESH%n_node; mesh%n_elem = n_elem
    mesh%coord = c_loc(hecMESH%node(1)); mesh%conn = c_loc(hecMESH%elem_node_item(1))
    nmat = size(fstrSOLID%materials)
    allocate(mats(nmat), emat(n_elem))
    ntmax = 1
    do i = 1, nmat
      if (fstrSOLID%materials(i)%mtype == -1) cycle
      if (isElastoplastic(fstrSOLID%materials(i)%mtype)) then
        if (getHardenType(fstrSOLID%materials(i)%mtype) == 1) ntmax = max(ntmax, fetch_TableRow(MC_YIELD, fstrSOLID%materials(i)%dict))
      endif
      if (fstrSOLID%materials(i)%mtype == VISCOELASTIC) ntmax = max(ntmax, fetch_TableRow(MC_VISCOELASTIC, fstrSOLID%materials(i)%dict))
    enddo
    if (allocated(tabs)) deallocate(tabs)
    allocate(tabs(2, ntmax, nmat))
    tabs = 0.d0
    do i = 1, nmat
      mats(i)%E = 1.d0; mats(i)%nu = 0.d0; mats(i)%plastic = 0; mats(i)%harden = 0; mats(i)%nlgeom = 0; mats(i)%ntab = 0
      mats(i)%plconst = 0.d0; mats(i)%tab = c_null_ptr; mats(i)%plconst4 = 0.d0
      if (fstrSOLID%materials(i)%mtype == -1) cycle
      mats(i)%E = fstrSOLID%materials(i)%variables(M_YOUNGS)
      mats(i)%nu = fstrSOLID%materials(i)%variables(M_POISSON)
      mats(i)%nlgeom = fstrSOLID%materials(i)%nlgeom_flag
      if (is_hyperelastic(fstrSOLID%materials(i)%mtype)) then      ! the material kind: 2 Neo-Hooke / Mooney-Rivlin, 3 Arruda-Boyce
        mats(i)%plastic = 2
        if (fstrSOLID%materials(i)%mtype == ARRUDABOYCE) mats(i)%plastic = 3
        mats(i)%plconst(1) = fstrSOLID%materials(i)%variables(M_PLCONST1)
        mats(i)%plconst(2) = fstrSOLID%materials(i)%variables(M_PLCONST2)
        mats(i)%plconst(3) = fstrSOLID%materials(i)%variables(M_PLCONST3)
      endif
      if (fstrSOLID%materials(i)%mtype == VISCOELASTIC) then      ! kind 7: the Prony rows (g, tau) as the reference holds them
        call fetch_Table(MC_VISCOELASTIC, fstrSOLID%materials(i)%dict, tbl, ierr_l)
        if (ierr_l) call fsd_fail('MC_VISCOELASTIC table')
        nt = tbl%tbrow
        tabs(1:2, 1:nt, i) = tbl%tbval(1:2, 1:nt)
        mats(i)%plastic = 7
        mats(i)%ntab = nt
        mats(i)%tab = c_loc(tabs(1, 1, i))
      endif
      if (fstrSOLID%materials(i)%mtype == NORTON) then            ! kind 8: A, n, m
        call fetch_Table(MC_NORTON, fstrSOLID%materials(i)%dict, tbl, ierr_l)
        if (ierr_l) call fsd_fail('MC_NORTON table')
        mats(i)%plastic = 8
        mats(i)%plconst(1:3) = tbl%tbval(1:3, 1)
      endif
      if (isElastoplastic(fstrSOLID%materials(i)%mtype)) then
        mats(i)%plastic = 1
        if (getYieldFunction(fstrSOLID%materials(i)%mtype) == 1) mats(i)%plastic = 4      ! Mohr-Coulomb: c, H, phi
        if (getYieldFunction(fstrSOLID%materials(i)%mtype) == 2) mats(i)%plastic = 5      ! Drucker-Prager: c, H, eta, xi
        mats(i)%plconst4 = fstrSOLID%materials(i)%variables(M_PLCONST4)
        mats(i)%harden = getHardenType(fstrSOLID%materials(i)%mtype)
        mats(i)%plconst(1) = fstrSOLID%materials(i)%variables(M_PLCONST1)
        mats(i)%plconst(2) = fstrSOLID%materials(i)%variables(M_PLCONST2)
        mats(i)%plconst(3) = fstrSOLID%materials(i)%variables(M_PLCONST3)
        if (mats(i)%harden == 1) then      ! MULTILINEAR: the MC_YIELD table as the reference holds it (tbval(1:2, 1:rows))
          call fetch_Table(MC_YIELD, fstrSOLID%materials(i)%dict, tbl, ierr_l)
          if (ierr_l) call fsd_fail('MC_YIELD table of a MULTILINEAR material')
          nt = tbl%tbrow
          tabs(1:2, 1:nt, i) = tbl%tbval(1:2, 1:nt)
          mats(i)%ntab = nt
          mats(i)%tab = c_loc(tabs(1, 1, i))
        endif
      endif
    enddo
    do icel = 1, n_elem
      emat(icel) = hecMESH%section%sect_mat_ID_item(hecMESH%section_ID(icel))
    enddo
    if (allocated(el_nq)) deallocate(el_nq, el_p0)
    allocate(el_nq(n_elem), el_p0(n_elem))
    el_nq = nl_nq
    if (nl_mixed .or. nl_fbar) then      ! elem_node_item holds the elements type by type: a group is a pointer into it (and into emat); 361: B-bar, or F-bar
      allocate(groups(hecMESH%n_elem_type))
      do itype = 1, hecMESH%n_elem_type
        first = hecMESH%elem_type_index(itype-1) + 1
        groups(itype)%etype = int(hecMESH%elem_type_item(itype), c_int32_t)
        groups(itype)%elemopt = 2
        if (nl_fbar) groups(itype)%elemopt = 4
        groups(itype)%n_elem = int(hecMESH%elem_type_index(itype) - hecMESH%elem_type_index(itype-1), c_int32_t)
        groups(itype)%conn = c_null_ptr
        groups(itype)%elem_mat = c_null_ptr
        if (groups(itype)%n_elem > 0) then
          groups(itype)%conn = c_loc(hecMESH%elem_node_item(hecMESH%elem_node_index(first-1) + 1))
          groups(itype)%elem_mat = c_loc(emat(first))
        endif
        nq = 8
        if (groups(itype)%etype /= 361) nq = c3_type_points(groups(itype)%etype)
        el_nq(first:hecMESH%elem_type_index(itype)) = nq
      enddo
    endif
    n_pt = 0      ! the per-point arrays: the elements in hecMESH's order, each with its own type's points
    do icel = 1, n_elem
      el_p0(icel) = n_pt
      n_pt = n_pt + el_nq(icel)
    enddo
    if (nl_mixed .or. nl_fbar) then      ! (a single-type F-bar mesh: one group, which makes the single-type context)
      ierr = fx_nl_init_groups(ctx, int(hecMESH%n_node, c_int32_t), hecMESH%node, int(size(groups), c_int32_t), groups, &
                               int(nmat, c_int32_t), mats)
      if (ierr /= 0) call fsd_fail('fx_nl_init_groups')
      deallocate(groups)
    else if (nl_etype == 361) then
      ierr = fx_nl_init_sections(ctx, mesh, int(nmat, c_int32_t), mats, emat)
      if (ierr /= 0) call fsd_fail('fx_nl_init_sections')
    else
      ierr = fx_nl_init_type(ctx, mesh, nl_etype, int(c3_type_nodes(nl_etype), c_int32_t), int(nmat, c_int32_t), mats, emat)
      if (ierr /= 0) call fsd_fail('fx_nl_init_type')
    endif
    deallocate(mats, emat)
    if (nl_thermal) call fsd_init_thermal(ctx, hecMESH, fstrSOLID)
    nl_hw = 0
    if (nl_timed) then
      ierr = fx_nl_get_history(ctx, c_null_ptr, nl_hw)
      if (ierr /= 0) call fsd_fail('fx_nl_get_history')
    endif
    if (allocated(b6)) deallocate(b6, bi)
    allocate(b6(6, n_pt), bi(n_pt))
    call fsd_push_state(ctx, fstrSOLID)
    ready = .true.
    the_ctx_saved = ctx
    if (fstr_cutback_is_on(fstrSOLID)) then    ! the state fstr_solve_NLGEOM.f90:84 saved on the host before the device had any
      ierr = fx_nl_snapshot(ctx, 0_c_int)
      if (ierr /= 0) call fsd_fail('fx_nl_snapshot')
    endif
  end subroutine fsd_init

  type(c_ptr) function the_device_ctx()
    the_device_ctx = the_ctx_saved
  end function the_device_ctx

  logical function fstr_cutback_is_on(fstrSOLID)       ! is_cutback_active of fstr_Cutback.f90:32-34
    type(fstr_solid), intent(in) :: fstrSOLID
    integer :: i
    fstr_cutback_is_on = .false.
    do i = 1, fstrSOLID%nstep_tot
      if (fstrSOLID%step_ctrl(i)%inc_type == stepAutoInc) fstr_cutback_is_on = .true.
    enddo
  end function fstr_cutback_is_on

  subroutine fsd_fail(what)
    character(len=*), intent(in) :: what
    write(*,'(a,a,a,a)') '#### libfistr_hip-E: device assembly binding: ', what, ': ', trim(fxb_error_text())
    call hecmw_abort(hecmw_comm_get_comm())
  end subroutine fsd_fail

  !> host quadrature-point history -> device (initial state, or a state read from a restart file)
  subroutine fsd_push_state(ctx, fstrSOLID)
    type(c_ptr), intent(in) :: ctx
    type(fstr_solid), intent(inout), target :: fstrSOLID
    type(fx_nl_state_view) :: sv
    integer(c_int) :: ierr
    integer :: icel, g, p
    real(c_double), allocatable, target :: s6(:,:), sb6(:,:), e6b(:,:), pl(:), fs(:), hw(:,:)
    integer :: nf
    allocate(s6(6, n_pt), sb6(6, n_pt), e6b(6, n_pt), pl(n_pt), fs(n_pt))
    bi = 0; fs = 0.d0
    do icel = 1, n_elem      ! every element with its own type's points, at the cumulative point offset
      do g = 1, el_nq(icel)
        p = el_p0(icel) + g
        b6(:, p)  = fstrSOLID%elements(icel)%gausses(g)%strain
        s6(:, p)  = fstrSOLID%elements(icel)%gausses(g)%stress
        e6b(:, p) = fstrSOLID%elements(icel)%gausses(g)%strain_bak
        sb6(:, p) = fstrSOLID%elements(icel)%gausses(g)%stress_bak
        pl(p)     = fstrSOLID%elements(icel)%gausses(g)%plstrain
        if (associated(fstrSOLID%elements(icel)%gausses(g)%istatus)) bi(p) = fstrSOLID%elements(icel)%gausses(g)%istatus(1)
        if (associated(fstrSOLID%elements(icel)%gausses(g)%fstatus)) fs(p) = fstrSOLID%elements(icel)%gausses(g)%fstatus(1)
      enddo
    enddo
    sv%stress = c_loc(s6(1,1)); sv%strain = c_loc(b6(1,1)); sv%stress_bak = c_loc(sb6(1,1)); sv%strain_bak = c_loc(e6b(1,1))
    sv%plstrain = c_loc(pl(1)); sv%fstat = c_loc(fs(1)); sv%istat = c_loc(bi(1))
    sv%unode = c_loc(fstrSOLID%unode(1)); sv%dunode = c_loc(fstrSOLID%dunode(1)); sv%qforce = c_loc(fstrSOLID%QFORCE(1))
    sv%latch = -1
    ierr = fx_nl_set_state(ctx, sv)
    if (ierr /= 0) call fsd_fail('fx_nl_set_state')
    if (nl_hw > 0) then      ! the whole fstatus(:) of the viscoelastic and NORTON points, [point][nl_hw], zero behind a shorter one
      allocate(hw(nl_hw, n_pt))
      hw = 0.d0
      do icel = 1, n_elem
        if (.not. timed_mtype(fstrSOLID%elements(icel)%gausses(1)%pMaterial%mtype)) cycle
        do g = 1, el_nq(icel)
          nf = min(size(fstrSOLID%elements(icel)%gausses(g)%fstatus), int(nl_hw))
          hw(1:nf, el_p0(icel) + g) = fstrSOLID%elements(icel)%gausses(g)%fstatus(1:nf)
        enddo
      enddo
      ierr = fx_nl_set_history(ctx, c_loc(hw(1,1)), nl_hw)
      if (ierr /= 0) call fsd_fail('fx_nl_set_history')
      deallocate(hw)
    endif
    deallocate(s6, sb6, e6b, pl, fs)
  end subroutine fsd_push_state

  logical function timed_mtype(mtype)
    integer, intent(in) :: mtype
    timed_mtype = (mtype == VISCOELASTIC .or. mtype == NORTON)
  end function timed_mtype

  !> ctime and tincr of the call in hand, as fstr_Newton hands them to fstr_StiffMatrix and fstr_UpdateNewton (tincr = 0 in a STATIC step)
  subroutine fsd_set_time(time, tincr)
    real(kind=kreal), intent(in) :: time, tincr
    nl_time = time
    nl_tincr = tincr
  end subroutine fsd_set_time

  subroutine fsd_apply_time(ctx)
    type(c_ptr), intent(in) :: ctx
    integer(c_int) :: ierr
    if (.not. nl_timed) return
    ierr = fx_nl_set_time(ctx, nl_time, nl_tincr)
    if (ierr /= 0) call fsd_fail('fx_nl_set_time')
  end subroutine fsd_apply_time

  !> fstr_StiffMatrix on the device; .false. = not covered, the caller runs the reference's routine.
  logical function fsd_stiffness(hecMESH, hecMAT, fstrSOLID)
    type(hecmwST_local_mesh), intent(in), target :: hecMESH
    type(hecmwST_matrix), intent(inout), target :: hecMAT
    type(fstr_solid), intent(inout), target :: fstrSOLID
    integer(c_int) :: ierr
    real(c_float) :: ms
    type(fx_mesh_view) :: mesh
    character(len=8) :: env
    integer :: elen, estat
    integer(kind=8) :: units
    fsd_stiffness = .false.
    fxb_matrix_on_device = .false.
    if (.not. fsd_eligible(hecMESH, hecMAT, fstrSOLID)) then
      if (.not. fsd_eligible_linear(hecMESH, hecMAT, fstrSOLID)) return
      if (.not. lin_ready) call fsd_init_linear(hecMESH, hecMAT, fstrSOLID)
      mesh%n_node = hecMESH%n_node; mesh%n_elem = hecMESH%n_elem
      mesh%coord = c_loc(hecMESH%node(1)); mesh%conn = c_loc(hecMESH%elem_node_item(1))
      if (lin_mixed) then
        ierr = fx_assemble_groups(fxb_context(hecMESH), int(hecMESH%n_node, c_int32_t), hecMESH%node, &
                                  int(size(lin_groups), c_int32_t), lin_groups, int(size(lin_E), c_int32_t), lin_E, lin_nu, &
                                  c_null_ptr, 0_c_int32_t, c_null_ptr, c_null_ptr, c_null_ptr, ms)
        if (ierr /= 0) call fsd_fail('fx_assemble_groups')
      else if (lin_etype == 361) then
        ierr = fx_assemble_c3d8_sections(fxb_context(hecMESH), mesh, int(size(lin_E), c_int32_t), lin_E, lin_nu, lin_emat, &
                                         lin_elemopt, c_null_ptr, 0_c_int32_t, c_null_ptr, c_null_ptr, c_null_ptr, ms)
        if (ierr /= 0) call fsd_fail('fx_assemble_c3d8_sections')
      else
        ierr = fx_assemble_c3(fxb_context(hecMESH), mesh, lin_etype, int(size(lin_E), c_int32_t), lin_E, lin_nu, lin_emat, &
                              c_null_ptr, 0_c_int32_t, c_null_ptr, c_null_ptr, c_null_ptr, ms)
        if (ierr /= 0) call fsd_fail('fx_assemble_c3')
      endif
      if (lin_mixed) then
        if (lin_update_on_device()) ierr = fx_update_groups_linear_prepare(fxb_context(hecMESH), int(size(lin_groups), c_int32_t), lin_groups)
      else if (lin_update_on_device()) then    ! the stress update follows the solve: pin its staging meanwhile (48 doubles per element unit)
        units = int(hecMESH%n_elem, 8)
        if (lin_etype /= 361) units = max(units, (units * 6 * c3_type_points(lin_etype) + 47) / 48)    ! 9 and 27 points need more
        ierr = fx_update_c3d8_linear_prepare(fxb_context(hecMESH), int(units, c_int32_t))
      endif
      fxb_matrix_on_device = .true.
      fsd_stiffness = .true.
      return
    endif
    if (.not. ready) call fsd_init(hecMESH, hecMAT, fstrSOLID)
    if (nl_thermal) then      ! fstrSOLID%temperature of this call (fstr_StiffMatrix.f90:72-73)
      ierr = fx_nl_set_temperature(fxb_context(hecMESH), fstrSOLID%temperature)
      if (ierr /= 0) call fsd_fail('fx_nl_set_temperature')
    endif
    call fsd_apply_time(fxb_context(hecMESH))
    ierr = fx_nl_stiffness_at(fxb_context(hecMESH), fstrSOLID%unode, fstrSOLID%dunode, ms)
    if (ierr /= 0) call fsd_fail('fx_nl_stiffness_at')
    fxb_matrix_on_device = .true.       ! from here to the solve: hecmw_mat_ass_bc records, hecmw_solve uses the resident matrix
    fsd_stiffness = .true.
  end function fsd_stiffness

  !> fstr_UpdateNewton on the device (QFORCE comes back, then the caller's halo update as fstr_Update.f90:284).
  logical function fsd_update_newton(hecMESH, fstrSOLID)
    type(hecmwST_local_mesh), intent(in) :: hecMESH
    type(fstr_solid), intent(inout), target :: fstrSOLID
    integer(c_int) :: ierr
    real(c_float) :: ms
    fsd_update_newton = .false.
    if (.not. ready) then
      if (lin_ready) fsd_update_newton = fsd_update_newton_linear(hecMESH, fstrSOLID)
      return
    endif
    if (nl_thermal) then      ! tt of fstr_Update.f90:101; the device's last_temp follows the host's through fx_nl_commit
      ierr = fx_nl_set_temperature(fxb_context(hecMESH), fstrSOLID%temperature)
      if (ierr /= 0) call fsd_fail('fx_nl_set_temperature')
    endif
    call fsd_apply_time(fxb_context(hecMESH))
    ierr = fx_nl_update_at(fxb_context(hecMESH), fstrSOLID%dunode, fstrSOLID%QFORCE, ms)
    if (ierr /= 0) call fsd_fail('fx_nl_update_at')
    call hecmw_update_3_R(hecMESH, fstrSOLID%QFORCE, hecMESH%n_node)
    fsd_update_newton = .true.
  end function fsd_update_newton

  !> fstr_cutback_save (load = 0) / fstr_cutback_load (load = 1) for the device's copy of the quadrature-point history.  Before the
  !> first fstr_StiffMatrix (fstr_solve_NLGEOM.f90:84 saves the initial state) there is nothing on the device yet: fsd_init will
  !> push the host's state, which is that very state, and takes the first snapshot itself.
  subroutine fsd_cutback(load)
    integer, intent(in) :: load
    integer(c_int) :: ierr
    if (.not. ready) return
    ierr = fx_nl_snapshot(the_device_ctx(), int(load, c_int))
    if (ierr /= 0) call fsd_fail('fx_nl_snapshot')
  end subroutine fsd_cutback

  !> fstr_UpdateNewton of a linear static deck (fsd_eligible_linear: TYPE=361, isotropic ELASTIC, the formulation of `ELEMOPT361`):
  !> UpdateST_C3D8IC / Update_C3D8Bbar / UPDATE_C3 for every element on the device from the total displacement unode + dunode
  !> (fstr_Update.f90:165 for IC; static_LIB_3d.f90:556 / static_LIB_C3D8.f90:258 for the others); strain and stress come back through
  !> the library's pinned staging into fstrSOLID%elements(:)%gausses(:), QFORCE into fstrSOLID%QFORCE, then the caller-side halo update
  !> of fstr_Update.f90:284.  HECMW_GPU_UPDATE=0 keeps the reference's element loop.
  logical function fsd_update_newton_linear(hecMESH, fstrSOLID)
    type(hecmwST_local_mesh), intent(in), target :: hecMESH
    type(fstr_solid), intent(inout), target :: fstrSOLID
    integer(c_int) :: ierr
    real(c_float) :: ms
    type(fx_mesh_view) :: mesh
    type(c_ptr) :: ps, pt
    real(c_double), pointer :: s6(:,:,:), t6(:,:,:)
    real(c_double), allocatable :: tot(:)
    character(len=8) :: env
    integer :: elen, estat, icel, g, nq, itype, first
    real(kind=kreal) :: t0
    type(c_ptr), allocatable :: gps(:), gpt(:)
    type, bind(C) :: fx_thermal_view
      type(c_ptr) :: temp, temp0
      real(c_double) :: ref_temp
      type(c_ptr) :: alpha
    end type fx_thermal_view
    interface
      integer(c_int) function fx_update_groups_linear_thermal(ctx, n_node, coord, n_group, groups, n_mat, E, nu, thermal, disp, &
          strain, stress, qforce, ms) bind(C, name='fx_update_groups_linear_thermal')
        import :: c_int, c_int32_t, c_ptr, c_double, c_float, fx_elem_group, fx_thermal_view
        type(c_ptr), value :: ctx
        integer(c_int32_t), value :: n_node, n_group, n_mat
        real(c_double), intent(in) :: coord(*), E(*), nu(*), disp(*)
        type(fx_elem_group), intent(in) :: groups(*)
        type(fx_thermal_view), intent(in) :: thermal
        type(c_ptr), intent(out) :: strain(*), stress(*)
        real(c_double), intent(inout) :: qforce(*)
        real(c_float), intent(out) :: ms
      end function fx_update_groups_linear_thermal
    end interface
    type(fx_thermal_view) :: tv
    real(c_double), allocatable, target :: tt0(:)
    fsd_update_newton_linear = .false.
    if (.not. lin_update_on_device()) return
    allocate(tot(3*hecMESH%n_node))
    tot(:) = fstrSOLID%unode(1:3*hecMESH%n_node) + fstrSOLID%dunode(1:3*hecMESH%n_node)
    mesh%n_node = hecMESH%n_node; mesh%n_elem = hecMESH%n_elem
    mesh%coord = c_loc(hecMESH%node(1)); mesh%conn = c_loc(hecMESH%elem_node_item(1))
    t0 = hecmw_Wtime()
    nq = 8
    if (lin_update_by_groups()) then ! every group's results come back in its own (6, nq, n_elem) block of the staging
      allocate(gps(size(lin_groups)), gpt(size(lin_groups)))
      if (lin_thermal) then          ! tt0 of fstr_Update.f90:92-102 for elastic materials: the initial condition, or 0
        allocate(tt0(hecMESH%n_node))
        tt0 = 0.d0
        if (hecMESH%hecmw_flag_initcon == 1) tt0(:) = hecMESH%node_init_val_item(1:hecMESH%n_node)
        tv%temp = c_loc(fstrSOLID%temperature(1)); tv%temp0 = c_loc(tt0(1))
        tv%ref_temp = ref_temp; tv%alpha = c_loc(lin_alpha(1))
        ierr = fx_update_groups_linear_thermal(fxb_context(hecMESH), int(hecMESH%n_node, c_int32_t), hecMESH%node, &
                                               int(size(lin_groups), c_int32_t), lin_groups, int(size(lin_E), c_int32_t), lin_E, &
                                               lin_nu, tv, tot, gps, gpt, fstrSOLID%QFORCE, ms)
        if (ierr /= 0) call fsd_fail('fx_update_groups_linear_thermal')
        deallocate(tt0)
      else
        ierr = fx_update_groups_linear(fxb_context(hecMESH), int(hecMESH%n_node, c_int32_t), hecMESH%node, &
                                       int(size(lin_groups), c_int32_t), lin_groups, int(size(lin_E), c_int32_t), lin_E, lin_nu, &
                                       tot, gps, gpt, fstrSOLID%QFORCE, ms)
        if (ierr /= 0) call fsd_fail('fx_update_groups_linear')
      endif
      deallocate(tot)
      call fsd_report('  of which the library call (uploads, kernel, strain / stress / QFORCE back)', hecmw_Wtime() - t0)
      call fsd_report('  of which the element kernel alone', real(ms, kreal) * 1.d-3)
      do itype = 1, size(lin_groups)
        if (lin_groups(itype)%n_elem < 1) cycle
        nq = 8
        if (lin_groups(itype)%etype /= 361) nq = c3_type_points(lin_groups(itype)%etype)
        first = hecMESH%elem_type_index(itype-1)
        call c_f_pointer(gps(itype), s6, [6, nq, int(lin_groups(itype)%n_elem)])
        call c_f_pointer(gpt(itype), t6, [6, nq, int(lin_groups(itype)%n_elem)])
        !$omp parallel do default(shared) private(icel, g)
        do icel = 1, lin_groups(itype)%n_elem
          do g = 1, nq
            fstrSOLID%elements(first + icel)%gausses(g)%strain(1:6) = s6(1:6, g, icel)
            fstrSOLID%elements(first + icel)%gausses(g)%stress(1:6) = t6(1:6, g, icel)
          enddo
        enddo
        !$omp end parallel do
      enddo
      deallocate(gps, gpt)
      call hecmw_update_3_R(hecMESH, fstrSOLID%QFORCE, hecMESH%n_node)
      fsd_update_newton_linear = .true.
      return
    endif
    if (lin_etype == 361) then
      ierr = fx_update_c3d8_linear(fxb_context(hecMESH), mesh, int(size(lin_E), c_int32_t), lin_E, lin_nu, lin_emat, lin_elemopt, &
                                   tot, ps, pt, fstrSOLID%QFORCE, ms)
      if (ierr /= 0) call fsd_fail('fx_update_c3d8_linear')
    else                             ! UPDATE_C3 at the type's quadrature points: 1 (341), 4 (342), 2 (351), 9 (352), 27 (362)
      nq = c3_type_points(lin_etype)
      ierr = fx_update_c3_linear(fxb_context(hecMESH), mesh, lin_etype, int(size(lin_E), c_int32_t), lin_E, lin_nu, lin_emat, &
                                 tot, ps, pt, fstrSOLID%QFORCE, ms)
      if (ierr /= 0) call fsd_fail('fx_update_c3_linear')
    endif
    deallocate(tot)
    call fsd_report('  of which the library call (uploads, kernel, strain / stress / QFORCE back)', hecmw_Wtime() - t0)
    call fsd_report('  of which the element kernel alone', real(ms, kreal) * 1.d-3)
    call c_f_pointer(ps, s6, [6, nq, hecMESH%n_elem])
    call c_f_pointer(pt, t6, [6, nq, hecMESH%n_elem])
    !$omp parallel do default(shared) private(icel, g)
    do icel = 1, hecMESH%n_elem
      do g = 1, nq
        fstrSOLID%elements(icel)%gausses(g)%strain(1:6) = s6(1:6, g, icel)
        fstrSOLID%elements(icel)%gausses(g)%stress(1:6) = t6(1:6, g, icel)
      enddo
    enddo
    !$omp end parallel do
    call hecmw_update_3_R(hecMESH, fstrSOLID%QFORCE, hecMESH%n_node)
    fsd_update_newton_linear = .true.
  end function fsd_update_newton_linear

  !> fstr_UpdateState on the device, then the history comes back to fstrSOLID%elements (results, restart files and whatever else
  !> of fistr1 reads it) -- once per sub-step, not per Newton iteration.
  logical function fsd_update_state(hecMESH, fstrSOLID, tincr)
    type(hecmwST_local_mesh), intent(in) :: hecMESH
    type(fstr_solid), intent(inout), target :: fstrSOLID
    real(kind=kreal), intent(in) :: tincr      ! fstr_UpdateState's: the two state updates of the time-dependent materials run under tincr > 0
    type(fx_nl_state_view) :: sv
    type(c_ptr) :: ctx
    integer(c_int) :: ierr
    integer :: icel, g, p, nf
    real(c_double), allocatable, target :: s6(:,:), pl(:), fs(:), hw(:,:)
    fsd_update_state = .false.
    if (.not. ready) return
    ctx = fxb_context(hecMESH)
    nl_tincr = tincr
    call fsd_apply_time(ctx)
    ierr = fx_nl_commit(ctx)      ! unode += dunode is the host's (fstr_Newton :156-158); the device does the same on its copy
    if (ierr /= 0) call fsd_fail('fx_nl_commit')
    if (associated(fstrSOLID%temperature)) then      ! the host's copy too (fstr_Update.f90:308-312): fstr_ass_load reads it for the thermal load
      fstrSOLID%last_temp(1:hecMESH%n_node) = fstrSOLID%temperature(1:hecMESH%n_node)
    endif
    allocate(s6(6, n_pt), pl(n_pt), fs(n_pt))
    sv%stress = c_loc(s6(1,1)); sv%strain = c_loc(b6(1,1)); sv%stress_bak = c_null_ptr; sv%strain_bak = c_null_ptr
    sv%plstrain = c_loc(pl(1)); sv%fstat = c_loc(fs(1)); sv%istat = c_loc(bi(1))
    sv%unode = c_null_ptr; sv%dunode = c_null_ptr; sv%qforce = c_null_ptr
    sv%latch = -1
    ierr = fx_nl_get_state(ctx, sv)
    if (ierr /= 0) call fsd_fail('fx_nl_get_state')
    do icel = 1, n_elem
      do g = 1, el_nq(icel)
        p = el_p0(icel) + g
        fstrSOLID%elements(icel)%gausses(g)%strain = b6(:, p)
        fstrSOLID%elements(icel)%gausses(g)%stress = s6(:, p)
        fstrSOLID%elements(icel)%gausses(g)%strain_bak = b6(:, p)     ! fstr_UpdateState :338-339
        fstrSOLID%elements(icel)%gausses(g)%stress_bak = s6(:, p)
        fstrSOLID%elements(icel)%gausses(g)%plstrain = pl(p)
        if (associated(fstrSOLID%elements(icel)%gausses(g)%istatus)) fstrSOLID%elements(icel)%gausses(g)%istatus(1) = bi(p)
        if (associated(fstrSOLID%elements(icel)%gausses(g)%fstatus)) fstrSOLID%elements(icel)%gausses(g)%fstatus(1) = fs(p)
      enddo
    enddo
    if (nl_hw > 0) then      ! the whole fstatus(:) back: result output, restart files and the host's cutback copies read it
      allocate(hw(nl_hw, n_pt))
      ierr = fx_nl_get_history(ctx, c_loc(hw(1,1)), nl_hw)
      if (ierr /= 0) call fsd_fail('fx_nl_get_history')
      do icel = 1, n_elem
        if (.not. timed_mtype(fstrSOLID%elements(icel)%gausses(1)%pMaterial%mtype)) cycle
        do g = 1, el_nq(icel)
          nf = min(size(fstrSOLID%elements(icel)%gausses(g)%fstatus), int(nl_hw))
          fstrSOLID%elements(icel)%gausses(g)%fstatus(1:nf) = hw(1:nf, el_p0(icel) + g)
        enddo
      enddo
      deallocate(hw)
    endif
    deallocate(s6, pl, fs)
    fsd_update_state = .true.
  end function fsd_update_state

end module fstr_device_hip
